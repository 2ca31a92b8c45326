"""inference.py --visualize on tests/golden/actaffordance_sample with the tiny synthetic model and a forced [SEG] answer (as
tests/test_smooth_cli_gpu.py runs it): the panels the scoring call draws on the device against tests/overlay_ref.py over the plain
run's written tree, and against the files route (evaluation.py --visualize). The runs are made once and shared."""
import io
import os
import re
import shutil
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/score_ref.py, tests/overlay_ref.py
import overlay_ref as O   # noqa: E402
import score_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu

SAMPLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "actaffordance_sample")


def _files(root):
    out = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(d, f)
            out[os.path.relpath(p, root)] = open(p, "rb").read()
    return out


def _png(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data) if isinstance(data, bytes) else data))


def _gray(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("L"))


def _leaves(bench):
    return [(s, l) for s in sorted(os.listdir(bench)) if os.path.isdir(os.path.join(bench, s)) for l in sorted(os.listdir(os.path.join(bench, s)))]


def _frame_size_copy(dst):
    """The sample with every mask taken to its frame's size (256 x 256): what --score_cropped scores against."""
    from PIL import Image
    shutil.copytree(SAMPLE, dst)
    for sub, leaf in _leaves(dst):
        folder = os.path.join(dst, sub, leaf)
        w, h = Image.open(os.path.join(folder, "inpainting.png")).size
        for name in os.listdir(folder):
            if name.startswith(("aff_", "obj_")):
                small = R.resample_on(_gray(os.path.join(folder, name)) > 0, (h, w))
                Image.fromarray(small.astype(np.uint8) * 255).save(os.path.join(folder, name))
    return str(dst)


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """Every CLI run of this module, once: {name: (report, stdout)} and the directories they wrote."""
    import contextlib
    import torch
    import haff  # noqa: F401
    from haff import inference, lisa
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    tmp = tmp_path_factory.mktemp("visualize")
    orig = lisa.LisaMI355.evaluate

    def evaluate(self, *a, **kw):
        """Random-init models never emit [SEG]; force one so the mask branch of the CLI runs."""
        B = a[2].shape[0]
        kw["forced_answer"] = torch.tensor([[5, self.cfg.seg_token_idx, self.cfg.eos_token_id]]).expand(B, -1)
        kw["max_new_tokens"] = 3
        return orig(self, *a, **kw)

    def run(name, tail, bench=SAMPLE):
        buf = io.StringIO()
        with contextlib.redirect_stdout(buf):
            rep = inference.main(["--synthetic", "tiny", "--benchmark-dir", bench, "--vis_save_path", str(tmp / name / "th"),
                                  "--image_size", "224", "--batch-size", "3"] + tail)
        return rep, buf.getvalue()
    out = {"tmp": tmp, "cropped_bench": _frame_size_copy(tmp / "bench256")}
    mp = pytest.MonkeyPatch()
    mp.setattr(lisa.LisaMI355, "evaluate", evaluate)
    try:
        out["plain"] = run("plain", ["--score"])
        out["panels"] = run("panels", ["--score_only", "--visualize", str(tmp / "D"), "--visualize_examples", "0"])
        out["dot"] = run("dot", ["--score_only", "--visualize", str(tmp / "Ddot"), "--visualize_caption", ".", "--visualize_examples", "0"])
        out["straddle_bench"], out["straddle_best"] = _straddling_copy(tmp / "bench02", str(tmp / "plain" / "th0.5"))
        out["dot02"] = run("dot02", ["--score_only", "--visualize", str(tmp / "Ddot02"), "--visualize_caption", ".", "--visualize_examples", "0"],
                           bench=out["straddle_bench"])
        out["two"] = run("two", ["--score_only", "--visualize", str(tmp / "D2"), "--visualize_examples", "2", "--visualize_threshold", "0.3"])
        out["cropped"] = run("cropped", ["--score_only", "--score_cropped", "--visualize", str(tmp / "Dcrop"), "--visualize_examples", "0"],
                             bench=out["cropped_bench"])
    finally:
        mp.undo()
    return out


def _straddling_copy(dst, tree):
    """The sample with its ground truth rewritten from the plain run's 0.5 tree `tree`, so that the IoUs straddle 0.2 whatever the
    random model predicts: the frame with the largest prediction gets that prediction as its ground truth (IoU 1), every other
    frame the complement of its prediction (IoU 0). Returns (path, (video, frame) of the IoU-1 frame)."""
    from PIL import Image
    shutil.copytree(SAMPLE, dst)
    preds = {}
    for sub, leaf in _leaves(dst):
        hands = [os.path.join(tree, sub, leaf, f"aff_{side}.png") for side in ("left", "right")]
        preds[sub, leaf] = np.logical_or.reduce([np.zeros((855, 855), bool)] + [R.resample_on(_gray(p) > 0, (855, 855))
                                                                                for p in hands if os.path.exists(p)])
    best = max(preds, key=lambda k: int(preds[k].sum()))
    assert preds[best].any()
    for (sub, leaf), pred in preds.items():
        folder = os.path.join(dst, sub, leaf)
        for side in ("left", "right"):
            if os.path.exists(os.path.join(folder, f"aff_{side}.png")):
                os.remove(os.path.join(folder, f"aff_{side}.png"))
        gt = pred if (sub, leaf) == best else ~pred
        Image.fromarray(gt.astype(np.uint8) * 255).save(os.path.join(folder, "aff_left.png"))
    return str(dst), best


def _printed_ious(text, name, names):
    """The `IoU for <label>: x` lines print_report wrote for threshold folder `name` (folders in sorted order, equal blocks)."""
    lines = re.findall(r"^IoU for (\S+): (\S+)$", text, flags=re.M)
    per = len(lines) // len(names)
    k = sorted(names).index(name)
    return dict(lines[k * per:(k + 1) * per])


def _expected_panel(bench, tree, sub, leaf, target_hw):
    """(benchmark overlay, prediction overlay, counts) of one frame from the written tree `tree`/<sub>/<leaf>/aff_*.png by the
    restatements: the exact resample of each written hand to the target, the ground truth as stored."""
    from PIL import Image
    frame = np.asarray(Image.open(os.path.join(bench, sub, leaf, "inpainting.png")).convert("RGB"))
    hw = frame.shape[:2] if target_hw is None else target_hw
    gts, prs = [], []
    for side in ("left", "right"):
        g, p = os.path.join(bench, sub, leaf, f"aff_{side}.png"), os.path.join(tree, sub, leaf, f"aff_{side}.png")
        gts.append(_gray(g) > 0 if os.path.exists(g) else None)
        prs.append(R.resample_on(_gray(p) > 0, hw) if os.path.exists(p) else None)
    union = lambda planes: np.logical_or.reduce([np.zeros(hw, bool)] + [m for m in planes if m is not None])   # noqa: E731
    gt, pr = union(gts), union(prs)
    counts = ((pr & gt).sum(), (pr | gt).sum(), pr.sum(), gt.sum())
    return O.overlay(frame, gts[0], gts[1]), O.overlay(frame, prs[0], prs[1]), counts


def test_panels_show_what_was_scored(dev, runs):
    """One panel per scored frame; each is overlay_ref over the plain run's 0.5 tree under draw_captions, and its IoU text is the
    report's per-frame IoU."""
    from haff import evaluation
    rep, text = runs["panels"]
    tmp = runs["tmp"]
    assert not os.path.exists(tmp / "panels")                                  # --score_only still writes no tree
    leaves = _leaves(SAMPLE)
    assert sorted(os.listdir(tmp / "D")) == sorted(f"{s}_{l}_concatenated.png" for s, l in leaves) and len(leaves) == 4
    names = [r["threshold"] for r in rep["per_threshold"]]
    printed = _printed_ious(text, "th0.5", names)
    drawn = 0
    for sub, leaf in leaves:
        bench_o, pred_o, counts = _expected_panel(SAMPLE, str(tmp / "plain" / "th0.5"), sub, leaf, (855, 855))
        iou = R.iou_iocm(counts)[0]
        assert printed[f"{sub}/{leaf}"] == f"{iou:.4f}"
        canvas = np.concatenate([bench_o, pred_o], axis=1)
        want = np.asarray(evaluation.draw_captions(canvas, evaluation.panel_captions(f"{sub}/{leaf}", "Aff-Ex", iou, bench_o.shape[1])))
        got = _png(str(tmp / "D" / f"{sub}_{leaf}_concatenated.png"))
        assert np.array_equal(got, want), (sub, leaf, int((got != want).sum()))
        drawn += int(counts[2] > 0)
    assert drawn                                                               # the model predicted something somewhere


def test_the_flag_changes_no_number_and_no_written_byte(dev, runs):
    plain, _ = runs["plain"]
    for name in ("panels", "dot", "two"):
        rep, _ = runs[name]
        assert [r["threshold"] for r in rep["per_threshold"]] == [r["threshold"] for r in plain["per_threshold"]]
        for g, w in zip(rep["per_threshold"], plain["per_threshold"]):
            assert {k: g[k] for k in ("count", "failed", "iou", "iocm")} == {k: w[k] for k in ("count", "failed", "iou", "iocm")}
        assert rep["mean_average_precision"] == plain["mean_average_precision"]
    want = R.score_tree(SAMPLE, str(runs["tmp"] / "plain"), hausdorff=False)      # the --score run without the flag: as before
    assert [(r["iou"], r["iocm"], r["count"]) for r in plain["per_threshold"]] == [(r["iou"], r["iocm"], r["count"]) for r in want["per_threshold"]]
    assert len(_files(runs["tmp"] / "plain")) >= 20


def test_caption_dot_and_the_example_count(dev, runs):
    """The caption "." writes the prediction overlay alone and only for frames above IoU 0.2; --visualize_examples 2 draws the first
    two scored frames in sorted order, at --visualize_threshold."""
    tmp = runs["tmp"]
    leaves = _leaves(SAMPLE)
    expect = {}
    for sub, leaf in leaves:
        _, pred_o, counts = _expected_panel(SAMPLE, str(tmp / "plain" / "th0.5"), sub, leaf, (855, 855))
        if R.iou_iocm(counts)[0] > 0.2:
            expect[f"{sub}_{leaf}.png"] = pred_o
    assert sorted(os.listdir(tmp / "Ddot")) == sorted(expect)
    for name, pred_o in expect.items():
        assert np.array_equal(_png(str(tmp / "Ddot" / name)), pred_o)
    # the same run against ground truth that puts one frame at IoU 1 and the others at 0: the 0.2 filter keeps exactly that one
    sub, leaf = runs["straddle_best"]
    ious = {}
    for s, l in leaves:
        _, pred_o, counts = _expected_panel(runs["straddle_bench"], str(tmp / "plain" / "th0.5"), s, l, (855, 855))
        ious[s, l] = R.iou_iocm(counts)[0]
        if (s, l) == (sub, leaf):
            assert np.array_equal(_png(str(tmp / "Ddot02" / f"{s}_{l}.png")), pred_o)
    assert ious[sub, leaf] == 1.0 and all(v == 0.0 for k, v in ious.items() if k != (sub, leaf)) and len(ious) == 4
    assert os.listdir(tmp / "Ddot02") == [f"{sub}_{leaf}.png"]
    rep, text = runs["dot02"]
    printed = _printed_ious(text, "th0.5", [r["threshold"] for r in rep["per_threshold"]])
    assert printed == {f"{s}/{l}": f"{v:.4f}" for (s, l), v in ious.items()}
    assert sorted(os.listdir(tmp / "D2")) == sorted(f"{s}_{l}_concatenated.png" for s, l in leaves[:2])
    sub, leaf = leaves[0]
    _, pred_o, _ = _expected_panel(SAMPLE, str(tmp / "plain" / "th0.3"), sub, leaf, (855, 855))
    got = _png(str(tmp / "D2" / f"{sub}_{leaf}_concatenated.png"))
    assert np.array_equal(got[40:, 256:], pred_o[40:])                         # below the captions: the 0.3 prediction


def test_cropped_panels_equal_the_files_route(dev, runs):
    """--score_cropped on the copy whose masks are at frame size: target and frame coincide (the identity map), the written
    predictions need no resize, and evaluation.py --visualize --cropped over the plain run's 0.5 tree writes the same files."""
    from haff import evaluation
    tmp = runs["tmp"]
    out = tmp / "files_route"
    done = evaluation.main(["--benchmark_folder", runs["cropped_bench"], "--comparison_folder", str(tmp / "plain" / "th0.5"),
                            "--cropped", "--visualize", "--visualize-dir", str(out), "--num-examples", "100"])
    theirs, ours = _files(out), _files(tmp / "Dcrop")
    assert len(done) == len(theirs) == 4 and sorted(theirs) == sorted(ours)
    for name in theirs:
        assert np.array_equal(_png(theirs[name]), _png(ours[name])), name
    assert theirs == ours                                                      # and the same PNG encoding
    rep, text = runs["cropped"]
    printed = _printed_ious(text, "th0.5", [r["threshold"] for r in rep["per_threshold"]])
    assert {k: v for k, v in printed.items()} == {label: f"{iou:.4f}" for label, iou, _ in done}
