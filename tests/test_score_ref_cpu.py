"""CPU side of the device scorer (csrc/mask_score.hip, haff.scoring): the numpy restatement tests/score_ref.py against
evaluation.py, the scorer's walk against evaluate_folders on the ActAffordance sample, the new CLI flags, the library's host
refusals (nothing is launched: device pointers are never dereferenced) and validate()'s batching with a stub model."""
import math
import os
import types

import numpy as np
import pytest
import torch

import haff  # noqa: F401
from haff import evaluation as ev

import score_ref as R

SAMPLE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "actaffordance_sample")
PAIRS = [((256, 256), (855, 855)), ((5, 7), (13, 11)), ((17, 13), (6, 5)), ((1, 1), (4, 3)), ((300, 400), (855, 855)),
         ((9, 9), (9, 9)), ((480, 640), (224, 224))]
BAND_CAP = 1e-4            # the share of target pixels the near-tie band may hold (a condition on the inputs, checked)


def _sample_planes():
    from PIL import Image
    out = []
    for d, _, fs in sorted(os.walk(SAMPLE)):
        for f in sorted(fs):
            if f.startswith(("aff_", "obj_")) and f.endswith(".png"):
                out.append(np.asarray(Image.open(os.path.join(d, f)).convert("L")) > 0)
    return out


def disc_union(hw, seed, n=3):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:hw[0], :hw[1]]
    m = np.zeros(hw, bool)
    for _ in range(n):
        cy, cx = rng.uniform(0, hw[0]), rng.uniform(0, hw[1])
        r = rng.uniform(0.1, 0.35) * max(min(hw), 2)
        m |= (yy + 0.5 - cy) ** 2 + (xx + 0.5 - cx) ** 2 < r * r
    return m


@pytest.fixture(scope="module")
def sample_planes():
    planes = _sample_planes()
    assert len(planes) == 11 and all(p.shape == (855, 855) for p in planes)
    return planes


@pytest.mark.parametrize("src_hw,dst_hw", PAIRS)
def test_integer_rule_equals_evaluation_outside_the_near_tie_band(sample_planes, src_hw, dst_hw):
    assert (4 * dst_hw[0] * dst_hw[1]) % 510 != 0                      # no exact tie exists for this pair
    sources = [R.resample_on(p, src_hw) for p in sample_planes]       # the sample's planes taken to the source size
    sources += [disc_union(src_hw, s) for s in range(6)]
    sources += [np.ones(src_hw, bool), np.zeros(src_hw, bool)]
    for k, bits in enumerate(sources):
        want = ev._resize_bilinear(bits.astype(np.uint8) * 255, (dst_hw[1], dst_hw[0])) > 0
        got = R.resample_on(bits, dst_hw)
        band = R.near_tie(bits, dst_hw)
        assert band.sum() <= BAND_CAP * band.size, (k, int(band.sum()))
        assert np.array_equal(got[~band], want[~band]), (k, int((got != want).sum()))
    if src_hw == dst_hw:
        assert all(np.array_equal(R.resample_on(b, dst_hw), b) for b in sources)   # equal sizes: the identity


def test_taps_are_the_half_pixel_bilinear_taps():
    for n_in, n_out in ((5, 13), (17, 6), (1, 4), (256, 855), (9, 9), (640, 224)):
        i0, i1, w0, w1 = R.axis_taps(n_in, n_out)
        src = np.maximum((np.arange(n_out) + 0.5) * n_in / n_out - 0.5, 0.0)
        assert np.array_equal(i0, np.minimum(np.floor(src).astype(int), n_in - 1))
        assert np.all(w0 + w1 == 2 * n_out) and np.all(i1 <= n_in - 1) and np.all(w1[i0 == n_in - 1] == 0)
        assert np.allclose(i0 * w0 + i1 * w1, np.minimum(src, n_in - 1) * 2 * n_out)


def test_gate_and_counts_rules():
    assert R.gate(None) == (True, True)
    assert R.gate([0.7, 0.1, 0.1, 0.1]) == (True, False) and R.gate([0.1, 0.7, 0.1, 0.1]) == (False, True)
    assert R.gate([0.1, 0.1, 0.7, 0.1]) == (True, True) and R.gate([0.4, 0.4, 0.1, 0.1]) == (True, False)   # a tie: the first
    assert R.gate([0.1, 0.2, 0.1, 0.1, 0.1, 0.9, 0.0, 0.0]) == (True, True)                                    # index 5: neither
    x = np.array([[1.0, -1.0], [np.nan, 0.0]], np.float32)
    gt = np.array([[1, 0], [9, 0]], np.uint8)
    counts, unions = R.score_frame(x, None, None, gt, None, None, None, [0.0, -2.0], (2, 2))
    assert unions[0].tolist() == [[1, 0], [0, 0]] and unions[1].tolist() == [[1, 1], [0, 1]]     # NaN is off, 0.0 > 0.0 is off
    assert counts.tolist() == [[1, 2, 1, 2], [1, 4, 3, 2]]
    counts, _ = R.score_frame(x, x, [0.0, 1.0, 0.0, 0.0], None, None, None, np.zeros((2, 2), np.uint8), [0.0], (2, 2))
    assert counts.tolist() == [[0, 0, 0, 0]]                                                       # left gated, right ANDed away


def _write(path, plane_bool):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(plane_bool.astype(np.uint8) * 255).save(path)


def test_score_tree_reproduces_evaluate_folders_on_the_sample(tmp_path, monkeypatch):
    """The object masks written as 256 x 256 predictions (folder `a`), and all-zero predictions (folder `b`, every frame failed)."""
    from PIL import Image
    monkeypatch.setattr(ev, "calculate_hausdorff", lambda a, b: (0.0, 0.0))   # count, failed and the counts are what is compared
    pred = tmp_path / "pred"
    for sub in sorted(os.listdir(SAMPLE)):
        if not os.path.isdir(os.path.join(SAMPLE, sub)):
            continue
        for leaf in sorted(os.listdir(os.path.join(SAMPLE, sub))):
            for side in ("left", "right"):
                op = os.path.join(SAMPLE, sub, leaf, f"obj_{side}.png")
                if os.path.exists(op):
                    small = R.resample_on(np.asarray(Image.open(op).convert("L")) > 0, (256, 256))
                    _write(str(pred / "a" / sub / leaf / f"aff_{side}.png"), small)
                    _write(str(pred / "b" / sub / leaf / f"aff_{side}.png"), np.zeros((256, 256), bool))
    want = ev.evaluate_folders(SAMPLE, str(pred), calc_map=True, verbose=False)
    got = R.score_tree(SAMPLE, str(pred), hausdorff=False)
    assert [r["threshold"] for r in got["per_threshold"]] == [r["threshold"] for r in want["per_threshold"]] == ["a", "b"]
    for g, w in zip(got["per_threshold"], want["per_threshold"]):
        assert (g["count"], g["failed"]) == (w["count"], w["failed"])
    assert want["per_threshold"][0]["count"] == 4 and want["per_threshold"][1]["failed"] == 4
    # per-frame integer counts against evaluation's own resize, within the frame's near-tie pixel count
    for th in ("a", "b"):
        for label, counts, ties in got["frames"][th]:
            gt = np.zeros((855, 855), bool)
            pr = np.zeros((855, 855), bool)
            for side in ("left", "right"):
                gp, pp = os.path.join(SAMPLE, label, f"aff_{side}.png"), os.path.join(str(pred), th, label, f"aff_{side}.png")
                if os.path.exists(gp):
                    gt |= np.asarray(Image.open(gp).convert("L")) > 0
                if os.path.exists(pp):
                    pr |= ev._resize_bilinear(np.asarray(Image.open(pp).convert("L")), (855, 855)) > 0
            theirs = np.array([(pr & gt).sum(), (pr | gt).sum(), pr.sum(), gt.sum()])
            assert ties <= BAND_CAP * 855 * 855 * 2 and np.all(np.abs(counts - theirs) <= ties), (th, label, counts, theirs, ties)
    # the skips of score_frame: intersection with a missing object plane drops the frame in both
    want_i = ev.evaluate_folders(SAMPLE, str(pred), calc_map=True, take_intersection=True, verbose=False)
    got_i = R.score_tree(SAMPLE, str(pred), take_intersection=True, hausdorff=False)
    assert [(r["count"], r["failed"]) for r in got_i["per_threshold"]] == [(r["count"], r["failed"]) for r in want_i["per_threshold"]]
    want_c = ev.evaluate_folders(SAMPLE, str(pred), calc_map=True, is_cropped=True, verbose=False)   # 855 masks against 256 targets
    got_c = R.score_tree(SAMPLE, str(pred), is_cropped=True)
    assert [r["count"] for r in got_c["per_threshold"]] == [r["count"] for r in want_c["per_threshold"]] == [0, 0]


def test_report_from_counts_is_evaluate_folders_arithmetic():
    from haff import scoring
    frames = [("v/1", np.array([[4, 28, 16, 16], [0, 16, 0, 16]]), [(1.0, 2.0), (3.0, 3.0)]),
              ("v/2", np.array([[0, 0, 0, 0], [9, 16, 9, 16]]), [(0.0, 0.0), (5.0, 6.0)])]
    res = scoring.report_from_frames(["x0.7", "x0.3"], frames, True)
    assert [r["threshold"] for r in res["per_threshold"]] == ["x0.3", "x0.7"]       # sorted folder names
    r3, r7 = res["per_threshold"]
    assert r7["iou"] == (4 / 28 + 0.0) / 2 and r7["iocm"] == (4 / 16 + 0.0) / 2 and r7["failed"] == 1 and r7["count"] == 2
    assert r3["iou"] == (0.0 + 9 / 16) / 2 and r3["iocm"] == (0.0 + 1.0) / 2 and r3["failed"] == 1
    assert (r7["directed_hd"], r7["hd"], r3["directed_hd"], r3["hd"]) == (0.5, 1.0, 4.0, 4.5)
    assert res["best"] is r3 and res["mean_average_precision"] == float(np.mean([r3["iocm"], r7["iocm"]]))
    bare = scoring.report_from_frames(["a"], [(f[0], f[1][:1], None) for f in frames], False)
    assert bare["best"]["hd"] is None and bare["best"]["directed_hd"] is None and bare["best"]["count"] == 2
    assert scoring.report_from_frames(["a"], [], False)["best"]["count"] == 0


def test_inference_score_flags():
    from haff import inference
    a = inference.parse_args(["--benchmark-dir", "b"])
    assert not (a.score or a.score_only or a.score_cropped or a.score_intersection or a.score_hausdorff)
    a = inference.parse_args(["--benchmark-dir", "b", "--score_only", "--score_cropped", "--score_intersection", "--score_hausdorff"])
    assert a.score and a.score_only and a.score_cropped and a.score_intersection and a.score_hausdorff
    assert inference.parse_args(["--benchmark-dir", "b", "--score"]).score_only is False
    for bad in (["--benchmark-dir", "b", "--score_cropped"], ["--benchmark-dir", "b", "--score_intersection"],
                ["--benchmark-dir", "b", "--score_hausdorff"], ["--score"], ["--score_only"]):
        with pytest.raises(SystemExit):
            inference.parse_args(bad)


def test_library_refuses_on_the_host():
    lib = haff.load_library()
    got, big = R.score_refusals(lib)
    assert all(v == -1 for v in got.values()), {k: v for k, v in got.items() if v != -1}
    assert all(v == -2 for v in big.values()), big


class _StubModel:
    """forward(inference=True)'s output dict from the batch alone: seeded logits at the label size, counting the calls."""

    def __init__(self):
        self.calls, self.sizes, self.outs = 0, [], []

    def eval(self):
        return self

    def train(self):
        return self

    def __call__(self, **batch):
        self.calls += 1
        gl, gr = torch.stack(batch["masks_list_left"], 0).float(), torch.stack(batch["masks_list_right"], 0).float()
        B = gl.shape[0]
        self.sizes.append(B)
        g = torch.Generator().manual_seed(100 + self.calls)
        out = {"pred_masks_left": torch.randn(gl.shape, generator=g), "pred_masks_right": torch.randn(gr.shape, generator=g),
               "pred_taxonomies": torch.softmax(3 * torch.randn((B, 1, 4), generator=g), -1), "gt_masks_left": gl, "gt_masks_right": gr}
        self.outs.append(out)
        return out


@pytest.mark.parametrize("vbs,n", [(2, 5), (1, 3), (8, 5)])
def test_validate_batches_equal_size_samples(monkeypatch, vbs, n):
    from haff import checkpoint, config as hcfg, ops, scoring, train_ds
    cfg = hcfg.tiny()
    ds = train_ds.SyntheticAffDataset(cfg, n, 777, (12, 10), inference=True)
    monkeypatch.setattr(scoring, "pack_frames", lambda frames: frames)

    def ref_score(frames, ths, device, out_counts=None):
        rows = [R.score_frame(f["left"].numpy(), f["right"].numpy(), f["taxonomy"].numpy(), f["gt_left"].numpy(), f["gt_right"].numpy(),
                              None, None, ths, f["target_hw"])[0] for f in frames]
        return torch.from_numpy(np.stack(rows).astype(np.int32))
    monkeypatch.setattr(ops, "score_masks", ref_score)
    model = _StubModel()
    args = types.SimpleNamespace(val_batch_size=vbs, model_max_length=575, conv_type="llava_v1")
    iou, iocm = train_ds.validate(model, ds, checkpoint.ByteTokenizer(cfg), args, 0, 1, torch.device("cpu"))
    assert model.calls == math.ceil(n / vbs) and sum(model.sizes) == n and max(model.sizes) == min(vbs, n)
    # the parent's host formulas, sample by sample in order, on the same forwards
    ious, iocms = [], []
    for out in model.outs:
        for b in range(out["pred_masks_left"].shape[0]):
            t = int(out["pred_taxonomies"][b][0].argmax())
            left, right = (out["pred_masks_left"][b][0] > 0).numpy(), (out["pred_masks_right"][b][0] > 0).numpy()
            if t == 1:
                left[:] = False
            if t == 0:
                right[:] = False
            pred = np.logical_or(left, right)
            gt = np.logical_or(out["gt_masks_left"][b][0].numpy() > 0, out["gt_masks_right"][b][0].numpy() > 0)
            ious.append(train_ds.calculate_iou(pred, gt))
            iocms.append(train_ds.calculate_iocm(gt, pred))
    m_iou, m_iocm = train_ds.AverageMeter("IoU"), train_ds.AverageMeter("IoCM")
    for a, b in zip(ious, iocms):
        m_iou.update(a)
        m_iocm.update(b)
    assert iou == m_iou.avg and iocm == m_iocm.avg


def test_validation_groups_split_on_a_size_change():
    from haff import train_ds
    sizes = [(4, 4), (4, 4), (4, 4), (6, 4), (4, 4), (4, 4)]
    fetch = lambda i: {"mask_hw": sizes[i], "i": i}   # noqa: E731
    groups = [[s["i"] for s in g] for g in train_ds.validation_groups(fetch, 0, 6, 2, raw=True)]
    assert groups == [[0, 1], [2], [3], [4, 5]]
    assert [[s["i"] for s in g] for g in train_ds.validation_groups(fetch, 1, 5, 8, raw=True)] == [[1, 2], [3], [4]]
