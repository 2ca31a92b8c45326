"""The overlay launch of haff_score_masks (score_vis_kernel, csrc/mask_score.hip) through ops.score_masks(vis=) against
tests/overlay_ref.py, byte for byte. Every canvas is pre-filled with 0xA5 and its rows are longer than the panel, so the bytes the
kernel must leave alone are compared too. Integer decisions and fp32 arithmetic that is exact for create_overlay's weights: the bar
is equality."""
import numpy as np
import pytest
import torch

import overlay_ref as O
import score_ref as R

pytestmark = pytest.mark.gpu

FILL = 0xA5


def thresholds():
    from haff import postprocess as P
    return [P.sigmoid_logit_threshold(t) for t in P.THRESHOLDS]


def discs(hw, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:hw[0], :hw[1]]
    m = np.zeros(hw, bool)
    for _ in range(3):
        cy, cx, r = rng.uniform(0, hw[0]), rng.uniform(0, hw[1]), rng.uniform(0.15, 0.4) * max(min(hw), 2)
        m |= (yy + 0.5 - cy) ** 2 + (xx + 0.5 - cx) ** 2 < r * r
    return (m * rng.integers(1, 256, hw)).astype(np.uint8)


def smooth_logits(hw, seed):
    """Logits that cross every threshold along region borders."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:hw[0], :hw[1]]
    a, b, c = rng.uniform(0.5, 3, 3)
    f = np.sin(a * yy / max(hw[0], 2) * 6 + c) + np.cos(b * xx / max(hw[1], 2) * 6) + 0.1 * rng.standard_normal(hw)
    return (2.5 * f).astype(np.float32)


def frame(src_hw, dst_hw, frame_hw, seed, tax=(0.1, 0.1, 0.7, 0.1), left=True, right=True, gt=(True, True), obj=(False, False)):
    f = {"left": smooth_logits(src_hw, seed) if left else None, "right": smooth_logits(src_hw, seed + 1) if right else None,
         "taxonomy": None if tax is None else np.asarray(tax, np.float32), "target_hw": dst_hw, "src_hw": src_hw}
    for k, side in enumerate(("left", "right")):
        f[f"gt_{side}"] = discs(dst_hw, seed + 10 + k) if gt[k] else None
        f[f"obj_{side}"] = discs(dst_hw, seed + 20 + k) if obj[k] else None
    f["rgb"] = np.random.default_rng(seed + 30).integers(0, 256, tuple(frame_hw) + (3,)).astype(np.uint8)
    return f


def run(frames, draw, ths, dev, pad=5, bench=True):
    """ONE ops.score_masks call over `frames`; draw = {frame index: t}. Returns (counts int64 [n, T, 4], {frame index: the whole
    canvas buffer uint8 [Hf, 6 Wf + pad]}): a side-by-side canvas whose rows are `pad` bytes longer than the two panels."""
    from haff import cvlite, ops, scoring
    packed, records, bufs = [], [], {}
    for i, f in enumerate(frames):
        d = {"target_hw": f["target_hw"], "src_hw": f["src_hw"]}
        for k in ("left", "right", "taxonomy", "gt_left", "gt_right", "obj_left", "obj_right"):
            d[k] = None if f[k] is None else torch.from_numpy(f[k]).to(dev)
        if i in draw:
            hf, wf = f["rgb"].shape[:2]
            stride = 6 * wf + pad
            buf = torch.full((hf, stride), FILL, dtype=torch.uint8, device=dev)
            out = [torch.as_strided(buf, (hf, wf, 3), (stride, 3, 1), k * 3 * wf) for k in (0, 1)]
            assert out[1].data_ptr() == out[0].data_ptr() + 3 * wf
            row = col = None
            if (hf, wf) != tuple(f["target_hw"]):
                row = torch.from_numpy(cvlite.nearest_indices(hf, f["target_hw"][0]).astype(np.int32)).to(dev)
                col = torch.from_numpy(cvlite.nearest_indices(wf, f["target_hw"][1]).astype(np.int32)).to(dev)
            records.append({"rgb": torch.from_numpy(f["rgb"]).to(dev), "row": row, "col": col, "t": draw[i],
                            "out": (out[0] if bench else None, out[1])})
            d["vis"] = len(records)
            bufs[i] = buf
        packed.append(d)
    counts = ops.score_masks(scoring.pack_frames(packed), ths, dev, vis=scoring.pack_vis(records) if records else None)
    return counts.cpu().numpy().astype(np.int64), {i: b.cpu().numpy() for i, b in bufs.items()}


def expected(f, th, pad=5, bench=True):
    hf, wf = f["rgb"].shape[:2]
    want = np.full((hf, 6 * wf + pad), FILL, np.uint8)
    b, p = O.panels(f, th, f["rgb"])
    if bench:
        want[:, :3 * wf] = b.reshape(hf, 3 * wf)
    want[:, 3 * wf:6 * wf] = p.reshape(hf, 3 * wf)
    return want


def check(f, t, dev, **kw):
    ths = thresholds()
    _, got = run([f], {0: t}, ths, dev, **kw)
    want = expected(f, ths[t], **kw)
    assert np.array_equal(got[0], want), int((got[0] != want).sum())
    return want


def test_every_byte_under_every_layer_pair(dev):
    """One 16 x 64 frame, identity map: pixel p holds the byte p mod 256 in all three channels under the on/off pair p div 256, for
    the prediction and for the benchmark layers."""
    p = np.arange(1024).reshape(16, 64)
    left_on, right_on = (p // 256) & 1 == 1, (p // 256) & 2 == 2
    f = {"left": np.where(left_on, 5.0, -5.0).astype(np.float32), "right": np.where(right_on, 5.0, -5.0).astype(np.float32),
         "taxonomy": None, "target_hw": (16, 64), "src_hw": (16, 64), "gt_left": left_on.astype(np.uint8) * 3,
         "gt_right": right_on.astype(np.uint8) * 255, "obj_left": None, "obj_right": None,
         "rgb": np.repeat((p % 256).astype(np.uint8)[:, :, None], 3, axis=2)}
    want = check(f, 2, dev)
    panel = want[:, 192:384].reshape(16, 64, 3)
    assert np.array_equal(panel, want[:, :192].reshape(16, 64, 3))          # the layers were made equal
    for pair in range(4):
        for c in range(3):
            seen = panel.reshape(4, 256, 3)[pair, :, c]
            assert np.array_equal(seen, O.blend_table(c)[:, pair & 1, pair >> 1])
    assert panel.reshape(4, 256, 3)[0, 1].tolist() == [0, 0, 0] and panel.reshape(4, 256, 3)[0, 3].tolist() == [2, 2, 2]
    assert panel.reshape(4, 256, 3)[1, 0].tolist() == [128, 0, 0] and panel.reshape(4, 256, 3)[2, 1].tolist() == [0, 128, 0]
    assert panel.reshape(4, 256, 3)[3, 255].tolist() == [255, 255, 128]


GEOMETRIES = [((5, 9), (13, 11), (7, 34)),       # tables down and up; the last thread of a row holds two pixels
              ((5, 9), (6, 7), (34, 29)),        # upscale tables; odd Wf: out[1] at an odd address, every row on the byte path
              ((5, 9), (13, 11), (13, 11)),      # identity map, Wf = 11: rows of 33 bytes
              ((21, 19), (45, 50), (300, 263))]  # more than one workgroup per frame (300 * 66 threads)


@pytest.mark.parametrize("src_hw,dst_hw,frame_hw", GEOMETRIES)
def test_geometry(dev, src_hw, dst_hw, frame_hw):
    check(frame(src_hw, dst_hw, frame_hw, 3), 2, dev)


def test_aligned_and_unaligned_rows(dev):
    """Wf = 36 with pad 4: every row of both canvases is word aligned (the word path); pad 5: three rows in four are not."""
    f = frame((5, 9), (13, 11), (7, 36), 4)
    check(f, 1, dev, pad=4)
    check(f, 1, dev, pad=5)


@pytest.mark.parametrize("t", range(5))
def test_each_threshold(dev, t):
    f = frame((17, 13), (31, 29), (23, 37), 5)
    check(f, t, dev)
    ths = thresholds()
    if t:
        assert not np.array_equal(expected(f, ths[t]), expected(f, ths[t - 1]))      # the threshold shows in the panel


@pytest.mark.parametrize("tax", [(0.7, 0.1, 0.1, 0.1), (0.1, 0.7, 0.1, 0.1), (0.1, 0.1, 0.7, 0.1), None])
def test_gate(dev, tax):
    check(frame((17, 13), (31, 29), (23, 37), 6, tax=tax), 2, dev)


@pytest.mark.parametrize("kw", [dict(obj=(True, False)), dict(obj=(False, True)), dict(left=False), dict(right=False),
                                dict(gt=(False, True)), dict(gt=(True, False)), dict(gt=(False, False))],
                         ids=["obj-left", "obj-right", "no-left", "no-right", "no-gt-left", "no-gt-right", "no-gt"])
def test_planes(dev, kw):
    check(frame((17, 13), (31, 29), (23, 37), 7, **kw), 2, dev)


def test_nan_logits_are_off(dev):
    f = frame((9, 9), (9, 9), (9, 9), 8)
    f["left"][:] = np.nan
    f["right"][::2] = np.nan
    want = check(f, 0, dev)
    f2 = frame((9, 9), (20, 23), (31, 30), 8)
    f2["left"][2:5] = np.nan
    check(f2, 4, dev)
    pred, _ = O.hand_bits(f, thresholds()[0])
    assert not pred[0].any() and not pred[1][::2].any() and want.any()


def test_benchmark_canvas_not_drawn(dev):
    f = frame((5, 9), (13, 11), (7, 34), 9)
    want = check(f, 2, dev, bench=False)
    assert (want[:, :3 * 34] == FILL).all()


def test_one_drawn_frame_in_a_batch_of_three_shapes(dev):
    ths = thresholds()
    frames = [frame((17, 13), (6, 5), (40, 41), 21, tax=(0.7, 0.1, 0.1, 0.1)), frame((66, 70), (131, 67), (50, 90), 22, obj=(True, True)),
              frame((5, 7), (13, 11), (13, 11), 23, tax=None, gt=(False, True))]
    counts, got = run(frames, {1: 3}, ths, dev)
    assert list(got) == [1] and np.array_equal(got[1], expected(frames[1], ths[3]))
    plain, none = run(frames, {}, ths, dev)
    assert none == {} and np.array_equal(counts, plain)                     # the counts of a call with overlays: bit-equal
    for k, f in enumerate(frames):
        assert np.array_equal(counts[k], R.score_frame(f["left"], f["right"], f["taxonomy"], f["gt_left"], f["gt_right"], f["obj_left"],
                                                       f["obj_right"], ths, f["target_hw"])[0])
    # all three drawn, the records in another order than the frames
    counts3, got3 = run(frames, {2: 0, 0: 4, 1: 3}, ths, dev)
    assert np.array_equal(counts3, plain) and np.array_equal(got3[1], got[1])
    assert np.array_equal(got3[0], expected(frames[0], ths[4])) and np.array_equal(got3[2], expected(frames[2], ths[0]))


def test_repeat_runs_are_bitwise_equal(dev):
    ths = thresholds()
    f = frame((21, 19), (45, 50), (300, 263), 3)
    a_c, a = run([f, f], {0: 2, 1: 2}, ths, dev)
    b_c, b = run([f, f], {0: 2, 1: 2}, ths, dev)
    assert np.array_equal(a_c, b_c) and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[0], a[1])


def test_other_weights_and_colours(dev):
    """Weights whose products are exact in fp32 (powers of two) but differ from create_overlay's, and other colours: the record's
    fields are read, not assumed."""
    from haff import ops, scoring
    ths = thresholds()
    f = frame((9, 9), (9, 9), (9, 9), 12)
    w = dict(alpha=(0.25, 0.5), beta=(1.0, 0.25), gamma=2.0, colors=((10, 200, 30), (255, 1, 77)))
    d = {k: (None if f[k] is None else torch.from_numpy(f[k]).to(dev)) for k in ("left", "right", "taxonomy", "gt_left", "gt_right")}
    d.update(target_hw=(9, 9), vis=1)
    canvas = torch.full((9, 18, 3), FILL, dtype=torch.uint8, device=dev)
    rec = dict(w, rgb=torch.from_numpy(f["rgb"]).to(dev), row=None, col=None, t=1, out=(canvas[:, :9], canvas[:, 9:]))
    ops.score_masks(scoring.pack_frames([d]), ths, dev, vis=scoring.pack_vis([rec]))
    b, p = O.panels(f, ths[1], f["rgb"], **w)
    assert np.array_equal(canvas.cpu().numpy(), np.concatenate([b, p], axis=1))


def test_weights_whose_products_round(dev):
    """alpha and beta that are no powers of two (0.3, 0.7): every product rounds in fp32, so a fused multiply-add, which skips one
    product's rounding, moves some bytes by one. Every frame byte under every layer pair, identity map, against the restatement's
    product-by-product arithmetic."""
    from haff import ops, scoring
    ths = thresholds()
    w = dict(alpha=(0.3, 0.3), beta=(0.7, 0.3), gamma=0.1, colors=((50, 200, 123), (50, 77, 255)))
    p = np.arange(1024).reshape(16, 64)
    left_on, right_on = (p // 256) & 1 == 1, (p // 256) & 2 == 2
    rgb = np.repeat((p % 256).astype(np.uint8)[:, :, None], 3, axis=2)
    f = {"left": np.where(left_on, 5.0, -5.0).astype(np.float32), "right": np.where(right_on, 5.0, -5.0).astype(np.float32),
         "taxonomy": None, "target_hw": (16, 64), "gt_left": left_on.astype(np.uint8), "gt_right": right_on.astype(np.uint8),
         "obj_left": None, "obj_right": None}
    # the case can tell: fusing the second blend's first product (fma(t1, alpha1, fl(b beta1))) changes a byte of this table
    f32, moved = np.float32, 0
    for t1 in range(256):
        for colour in (50, 77, 255):
            pb = float(f32(f32(colour) * f32(0.3)))
            fused = float(f32(float(t1) * float(f32(0.3)) + pb))
            moved += O.blend_byte(t1, 0.3, colour, 0.3, 0.1) != max(0, min(255, round(float(f32(f32(fused) + f32(0.1))))))
    assert moved > 0
    d = {k: (None if f[k] is None else torch.from_numpy(f[k]).to(dev)) for k in ("left", "right", "gt_left", "gt_right")}
    d.update(target_hw=(16, 64), taxonomy=None, vis=1)
    canvas = torch.full((16, 128, 3), FILL, dtype=torch.uint8, device=dev)
    rec = dict(w, rgb=torch.from_numpy(rgb).to(dev), row=None, col=None, t=0, out=(canvas[:, :64], canvas[:, 64:]))
    ops.score_masks(scoring.pack_frames([d]), ths, dev, vis=scoring.pack_vis([rec]))
    b, pr = O.panels(f, ths[0], rgb, **w)
    got = canvas.cpu().numpy()
    want = np.concatenate([b, pr], axis=1)
    assert np.array_equal(got, want), int((got != want).sum())
    for c in range(3):
        assert np.array_equal(pr.reshape(4, 256, 3)[3, :, c], O.blend_table(c, **w)[:, 1, 1])
