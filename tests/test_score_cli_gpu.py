"""inference.py --score / --score_only and train_ds.validate on the device scorer (haff.scoring, csrc/mask_score.hip): the tiny
synthetic model with a forced [SEG] answer, as tests/test_cli_gpu.py runs it, on tests/golden/actaffordance_sample."""
import os
import re
import shutil

import numpy as np
import pytest

import score_ref as R

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


def _same_report(got, want, fields):
    assert [r["threshold"] for r in got["per_threshold"]] == [r["threshold"] for r in want["per_threshold"]]
    for g, w in zip(got["per_threshold"], want["per_threshold"]):
        for k in ("count", "failed") + fields:
            assert g[k] == w[k], (g["threshold"], k, g[k], w[k])
    assert got["best"]["threshold"] == want["best"]["threshold"]
    assert got["mean_average_precision"] == want["mean_average_precision"]


def test_score_equals_the_reference_walk_over_the_written_tree(dev, tmp_path, forced, capsys, monkeypatch):
    """--score changes no written byte; its report is score_ref.score_tree's on those PNGs (IoU and IoCM exactly: the same integers),
    with evaluate_folders' count and failed; --score_only writes nothing and reports the same IoU and IoCM."""
    from haff import evaluation
    assert _run([], SAMPLE, str(tmp_path / "plain" / "th")) is None
    capsys.readouterr()
    rep = _run(["--score"], SAMPLE, str(tmp_path / "scored" / "th"))
    text = capsys.readouterr().out
    plain, scored = _files(tmp_path / "plain"), _files(tmp_path / "scored")
    assert len(plain) >= 20 and plain == scored
    want = R.score_tree(SAMPLE, str(tmp_path / "scored"), hausdorff=False)
    _same_report(rep, want, ("iou", "iocm", "hd", "directed_hd"))
    assert rep["best"]["hd"] is None and [r["count"] for r in rep["per_threshold"]] == [4] * 5
    assert f"mean average precision: {rep['mean_average_precision']}" in text and "Hausdorff-Distance: not computed" in text
    assert f"Best performing threshold was {rep['best']['threshold']}" in text and "IoU for P14_05/0001413:" in text
    monkeypatch.setattr(evaluation, "calculate_hausdorff", lambda a, b: (0.0, 0.0))   # only its count and failed are compared
    theirs = evaluation.evaluate_folders(SAMPLE, str(tmp_path / "scored"), calc_map=True, verbose=False)
    assert [(r["count"], r["failed"]) for r in rep["per_threshold"]] == [(r["count"], r["failed"]) for r in theirs["per_threshold"]]
    only = _run(["--score_only"], SAMPLE, str(tmp_path / "none" / "th"))
    assert not os.path.exists(tmp_path / "none")
    _same_report(only, rep, ("iou", "iocm", "hd", "directed_hd"))
    # --score_intersection: the frames whose written hand has no obj_<side>.png leave the count, as in evaluate_folders
    inter = _run(["--score_only", "--score_intersection"], SAMPLE, str(tmp_path / "scored" / "th"))
    want_i = R.score_tree(SAMPLE, str(tmp_path / "scored"), take_intersection=True, hausdorff=False)
    _same_report(inter, want_i, ("iou", "iocm"))
    theirs_i = evaluation.evaluate_folders(SAMPLE, str(tmp_path / "scored"), calc_map=True, take_intersection=True, verbose=False)
    assert [(r["count"], r["failed"]) for r in inter["per_threshold"]] == [(r["count"], r["failed"]) for r in theirs_i["per_threshold"]]


def test_score_hausdorff_equals_the_reference_walk(dev, tmp_path, forced, capsys):
    """--score --score_hausdorff on two leaf folders of the sample (one per video: the Python contour walk costs about a second per
    855 x 855 plane, here and in the reference walk): the same PNG bytes, and a report equal to score_tree's in every field."""
    bench = tmp_path / "bench"
    for sub, leaf in (("P14_05", "0001413"), ("8f91bc0d-9ce7-4b31-aba7-dd59791917df", "00000029")):
        shutil.copytree(os.path.join(SAMPLE, sub, leaf), bench / sub / leaf)
    _run([], str(bench), str(tmp_path / "plain" / "th"))
    rep = _run(["--score", "--score_hausdorff"], str(bench), str(tmp_path / "scored" / "th"))
    text = capsys.readouterr().out
    assert _files(tmp_path / "plain") == _files(tmp_path / "scored")
    want = R.score_tree(str(bench), str(tmp_path / "scored"), hausdorff=True)
    _same_report(rep, want, ("iou", "iocm", "hd", "directed_hd"))
    assert rep["best"]["hd"] is not None and f"Hausdorff-Distance: {rep['best']['hd']}" in text
    import threading
    assert not [t for t in threading.enumerate() if t.name.startswith("haff-hausdorff")]     # the worker ended with the run


@pytest.mark.parametrize("vbs", [1, 2])
def test_validate_prints_the_host_formulas_numbers(dev, tmp_path, capsys, monkeypatch, vbs):
    """train_ds.main --eval_only on the tiny synthetic trainer: the printed IoU / IoCM are the old host formulas' (recomputed here
    from the very forward(inference=True) outputs validate() scored), and each sample's integer counts equal the host's counts."""
    import haff  # noqa: F401
    from haff import ops, train_ds
    outs, counts = [], []
    orig_frames, orig_score = train_ds.validation_frames, ops.score_masks

    def frames_spy(out):
        outs.append({k: out[k].detach().float().cpu() for k in ("pred_masks_left", "pred_masks_right", "pred_taxonomies",
                                                                 "gt_masks_left", "gt_masks_right")})
        return orig_frames(out)

    def score_spy(*a, **kw):
        c = orig_score(*a, **kw)
        counts.append(c)
        return c
    monkeypatch.setattr(train_ds, "validation_frames", frames_spy)
    monkeypatch.setattr(ops, "score_masks", score_spy)
    train_ds.main(["--synthetic", "tiny", "--eval_only", "--val_samples", "5", "--val_batch_size", str(vbs), "--mask_hw", "61", "47",
                   "--log_base_dir", str(tmp_path / "runs"), "--exp_name", "v"])
    text = capsys.readouterr().out
    assert [o["pred_masks_left"].shape[0] for o in outs] == ([1] * 5 if vbs == 1 else [2, 2, 1])
    iou_m, iocm_m = train_ds.AverageMeter("IoU"), train_ds.AverageMeter("IoCM")
    host_counts = []
    for o in outs:
        for b in range(o["pred_masks_left"].shape[0]):
            t = int(o["pred_taxonomies"][b][0].argmax())
            left, right = (o["pred_masks_left"][b][0] > 0).numpy(), (o["pred_masks_right"][b][0] > 0).numpy()
            if t == 1:
                left[:] = False
            if t == 0:
                right[:] = False
            pred = np.logical_or(left, right)
            gt = np.logical_or(o["gt_masks_left"][b][0].numpy() > 0, o["gt_masks_right"][b][0].numpy() > 0)
            iou_m.update(train_ds.calculate_iou(pred, gt))
            iocm_m.update(train_ds.calculate_iocm(gt, pred))
            host_counts.append([int((pred & gt).sum()), int((pred | gt).sum()), int(pred.sum()), int(gt.sum())])
    got = np.concatenate([c.cpu().numpy().reshape(-1, 4) for c in counts])
    assert got.tolist() == host_counts
    assert any(c[2] > 0 for c in host_counts) and any(c[3] > 0 for c in host_counts)
    m = re.search(r"IoU: ([0-9.]+), IoCM: ([0-9.]+)", text)
    assert m and (m.group(1), m.group(2)) == (f"{iou_m.avg:.4f}", f"{iocm_m.avg:.4f}")
