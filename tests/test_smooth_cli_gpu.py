"""inference.py --smooth_masks on tests/golden/actaffordance_sample with the tiny synthetic model and a forced [SEG] answer (as
tests/test_score_cli_gpu.py runs it): the device route against the files route — the plain run's tree, then smooth.py over a copy."""
import os
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/score_ref.py, tests/contours_ref.py
import contours_ref as C   # noqa: E402
import score_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu

SAMPLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "actaffordance_sample")


@pytest.fixture
def forced(monkeypatch):
    """Random-init models never emit [SEG]; force one so the mask branch of the CLI runs."""
    import torch
    import haff  # noqa: F401
    from haff import lisa
    orig = lisa.LisaMI355.evaluate

    def evaluate(self, *a, **kw):
        B = a[2].shape[0]
        kw["forced_answer"] = torch.tensor([[5, self.cfg.seg_token_idx, self.cfg.eos_token_id]]).expand(B, -1)
        kw["max_new_tokens"] = 3
        return orig(self, *a, **kw)
    monkeypatch.setattr(lisa.LisaMI355, "evaluate", evaluate)


def _files(root):
    out = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def _run(argv_tail, bench, vis):
    from haff import inference
    return inference.main(["--synthetic", "tiny", "--benchmark-dir", bench, "--vis_save_path", vis, "--image_size", "224",
                           "--batch-size", "3"] + argv_tail)


def _same_report(got, want, fields=("iou", "iocm", "hd", "directed_hd")):
    assert [r["threshold"] for r in got["per_threshold"]] == [r["threshold"] for r in want["per_threshold"]]
    for g, w in zip(got["per_threshold"], want["per_threshold"]):
        for k in ("count", "failed") + fields:
            assert g[k] == w[k], (g["threshold"], k, g[k], w[k])
    assert got["best"]["threshold"] == want["best"]["threshold"]
    assert got["mean_average_precision"] == want["mean_average_precision"]


def _smoothed_copy(src, dst, args):
    from haff import smooth
    shutil.copytree(src, dst)
    assert smooth.main(["--input_dir", str(dst)] + args) == len(_files(src))
    return _files(dst)


def _planes(files):
    from PIL import Image
    import io
    return {k: np.asarray(Image.open(io.BytesIO(v))) for k, v in files.items()}


@pytest.mark.timeout(600)
def test_smooth_masks_equals_the_files_route(dev, tmp_path, forced):
    """--smooth_masks writes, byte for byte, what smooth.py leaves of the plain run's tree; --score reports score_tree's numbers on
    that smoothed tree and --score_only the same without writing; --write_records holds the contours of the smoothed planes; the
    same with --smooth_threshold 0.25 against smooth.py --threshold 0.25."""
    import torch
    assert _run([], SAMPLE, str(tmp_path / "plain" / "th")) is None
    plain = _files(tmp_path / "plain")
    assert len(plain) >= 20
    want = _smoothed_copy(tmp_path / "plain", tmp_path / "files", [])
    # not vacuous: the smoothing changes pixels of written planes, and leaves something on
    before, after = _planes(plain), _planes(want)
    changed = sum(int((before[k] != after[k]).sum()) for k in before)
    assert changed > 0 and any(p.any() for p in after.values())
    assert all(set(np.unique(p).tolist()) <= {0, 255} and p.dtype == np.uint8 for p in after.values())

    records = str(tmp_path / "records.pt")
    rep = _run(["--smooth_masks", "--score", "--write_records", records, "--records_threshold", "0.3"], SAMPLE,
               str(tmp_path / "device" / "th"))
    got = _files(tmp_path / "device")
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], k
    ref = R.score_tree(SAMPLE, str(tmp_path / "files"), hausdorff=False)
    _same_report(rep, ref)
    assert [r["count"] for r in rep["per_threshold"]] == [4] * 5

    only = _run(["--smooth_masks", "--score_only"], SAMPLE, str(tmp_path / "none" / "th"))
    assert not os.path.exists(tmp_path / "none")
    _same_report(only, rep)

    # the records: every contour of the smoothed plane at the records threshold (the host walk is slow: two hands are walked)
    recs = torch.load(records, weights_only=False)
    assert len(recs) == 4
    leaves = sorted((sub, leaf) for sub in os.listdir(SAMPLE) if os.path.isdir(os.path.join(SAMPLE, sub))
                    for leaf in os.listdir(os.path.join(SAMPLE, sub)))
    walked = 0
    for rec, (sub, leaf) in zip(recs, leaves):
        for side, blank in (("left", 1), ("right", 0)):
            key = os.path.join("th0.3", sub, leaf, f"aff_{side}.png")
            assert (key in after) == (rec["taxonomy"] != blank), (key, rec["taxonomy"])
            if key in after and walked < 2:
                assert rec["masks"]["aff_" + side] == [c.reshape(-1, 2).tolist() for c in C.contours(after[key])], key
                walked += 1
    assert walked == 2

    want25 = _smoothed_copy(tmp_path / "plain", tmp_path / "files25", ["--threshold", "0.25"])
    assert want25 != want
    rep25 = _run(["--smooth_masks", "--smooth_threshold", "0.25", "--score"], SAMPLE, str(tmp_path / "device25" / "th"))
    got25 = _files(tmp_path / "device25")
    assert sorted(got25) == sorted(want25)
    for k in want25:
        assert got25[k] == want25[k], k
    _same_report(rep25, R.score_tree(SAMPLE, str(tmp_path / "files25"), hausdorff=False))
