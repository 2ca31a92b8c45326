"""haff_score_masks (csrc/mask_score.hip) through ops.score_masks against tests/score_ref.py: counts and union planes equal byte
for byte. Integer work, so the bar is equality: the reference is the exact rule itself, restated in numpy."""
import numpy as np
import pytest
import torch

import score_ref as R

pytestmark = pytest.mark.gpu

# (source, target): up, down, width 1, widths that are no multiple of 4 or 64, equal sizes, the benchmark's 256 -> 855
PAIRS = [((5, 7), (13, 11)), ((17, 13), (6, 5)), ((1, 1), (4, 3)), ((300, 400), (855, 855)), ((9, 9), (9, 9)),
         ((480, 640), (224, 224)), ((3, 1), (7, 9)), ((66, 70), (131, 67)), ((256, 256), (855, 855))]


def thresholds():
    from haff import postprocess as P
    return [P.sigmoid_logit_threshold(t) for t in P.THRESHOLDS] + [0.0]


def discs(hw, seed):
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:hw[0], :hw[1]]
    m = np.zeros(hw, bool)
    for _ in range(3):
        cy, cx, r = rng.uniform(0, hw[0]), rng.uniform(0, hw[1]), rng.uniform(0.1, 0.35) * max(min(hw), 2)
        m |= (yy + 0.5 - cy) ** 2 + (xx + 0.5 - cx) ** 2 < r * r
    return (m * rng.integers(1, 256, hw)).astype(np.uint8)        # on where > 0: any non-zero byte


def smooth_logits(hw, seed):
    """Logits that cross every threshold along region borders (white noise would put a border at every pixel)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:hw[0], :hw[1]]
    a, b, c = rng.uniform(0.5, 3, 3)
    f = np.sin(a * yy / max(hw[0], 2) * 6 + c) + np.cos(b * xx / max(hw[1], 2) * 6) + 0.1 * rng.standard_normal(hw)
    return (2.5 * f).astype(np.float32)


def frame(src_hw, dst_hw, seed, tax=(0.1, 0.1, 0.7, 0.1), left=True, right=True, gt=(True, True), obj=(False, False)):
    f = {"left": smooth_logits(src_hw, seed) if left else None, "right": smooth_logits(src_hw, seed + 1) if right else None,
         "taxonomy": None if tax is None else np.asarray(tax, np.float32), "target_hw": dst_hw, "src_hw": src_hw}
    for k, side in enumerate(("left", "right")):
        f[f"gt_{side}"] = discs(dst_hw, seed + 10 + k) if gt[k] else None
        f[f"obj_{side}"] = discs(dst_hw, seed + 20 + k) if obj[k] else None
    return f


def reference(f, ths):
    return R.score_frame(f["left"], f["right"], f["taxonomy"], f["gt_left"], f["gt_right"], f["obj_left"], f["obj_right"], ths,
                         f["target_hw"])


def _odd(plane, dev):
    """The plane at an address that is 1 mod 4: the byte path of the quad loads."""
    buf = torch.empty((plane.size + 5,), dtype=torch.uint8, device=dev)
    v = buf[1:1 + plane.size].view(plane.shape)
    v.copy_(torch.from_numpy(plane))
    assert v.data_ptr() % 4 == 1 and v.is_contiguous()
    return v


def run(frames, ths, dev, want_union=True, odd=False):
    """frames of numpy planes -> (counts int64 [n, T, 4], [unions uint8 [T, Hb, Wb]]) from ONE launch."""
    from haff import ops, scoring
    packed = []
    for f in frames:
        d = {"target_hw": f["target_hw"], "src_hw": f["src_hw"]}
        for k in ("left", "right", "taxonomy"):
            d[k] = None if f[k] is None else torch.from_numpy(f[k]).to(dev)
        for k in ("gt_left", "gt_right", "obj_left", "obj_right"):
            d[k] = None if f[k] is None else (_odd(f[k], dev) if odd else torch.from_numpy(f[k]).to(dev))
        if want_union:
            d["out"] = torch.full((len(ths),) + tuple(f["target_hw"]), 7, dtype=torch.uint8, device=dev)   # every byte is written
        packed.append(d)
    counts = ops.score_masks(scoring.pack_frames(packed), ths, dev)
    return counts.cpu().numpy().astype(np.int64), [d["out"].cpu().numpy() for d in packed] if want_union else None


_REF = {}


def pair_case(i):
    """The frame of PAIRS[i] and its reference, computed once for the tests that share it."""
    if i not in _REF:
        f = frame(PAIRS[i][0], PAIRS[i][1], 40 + i)
        _REF[i] = (f, reference(f, thresholds()))
    return _REF[i]


@pytest.mark.parametrize("i", range(len(PAIRS)))
def test_sizes(dev, i):
    f, (want_c, want_u) = pair_case(i)
    counts, unions = run([f], thresholds(), dev)
    assert np.array_equal(unions[0], want_u), int((unions[0] != want_u).sum())
    assert np.array_equal(counts[0], want_c), (counts[0], want_c)
    assert want_c[:, 2].max() > 0 or PAIRS[i][0] == (1, 1)       # the case predicts something


@pytest.mark.parametrize("tax,n_open", [((0.7, 0.1, 0.1, 0.1), "left"), ((0.1, 0.7, 0.1, 0.1), "right"), ((0.1, 0.1, 0.7, 0.1), "both"),
                                         ((0.1, 0.1, 0.1, 0.7), "both"), ((0.1, 0.2, 0.3, 0.1, 0.0, 0.9, 0.0, 0.0), "both"),
                                         ((0.2, 0.9, 0.3, 0.1, 0.95, 0.0, 0.0, 0.0), "both"),
                                         ((0.4, 0.4, 0.1, 0.1), "left"), ((0.1, 0.4, 0.4, 0.1), "right"), (None, "both")])
def test_gate(dev, tax, n_open):
    ths = [0.0, 0.5]
    f = frame((17, 13), (31, 29), 3, tax=tax)
    want_c, want_u = reference(f, ths)
    counts, unions = run([f], ths, dev)
    assert np.array_equal(unions[0], want_u) and np.array_equal(counts[0], want_c)
    only = {"left": dict(right=False), "right": dict(left=False), "both": {}}[n_open]
    alone = frame((17, 13), (31, 29), 3, tax=None, **only)     # the gate's effect, stated without the gate
    assert np.array_equal(reference(alone, ths)[1], want_u)


@pytest.mark.parametrize("left,right,gt,obj", [(False, True, (True, True), (False, False)), (True, False, (True, True), (False, False)),
                                                (False, False, (True, True), (False, False)), (True, True, (False, True), (False, False)),
                                                (True, True, (True, False), (False, False)), (True, True, (False, False), (False, False)),
                                                (True, True, (True, True), (True, True)), (True, True, (True, True), (True, False)),
                                                (True, True, (True, True), (False, True))])
@pytest.mark.parametrize("odd", [False, True])
def test_planes(dev, left, right, gt, obj, odd):
    ths = thresholds()
    f = frame((21, 19), (45, 50), 5, left=left, right=right, gt=gt, obj=obj)
    want_c, want_u = reference(f, ths)
    counts, unions = run([f], ths, dev, odd=odd)
    assert np.array_equal(unions[0], want_u) and np.array_equal(counts[0], want_c)
    counts_only, _ = run([f], ths, dev, want_union=False, odd=odd)          # no output plane: the same counts
    assert np.array_equal(counts_only[0], want_c)


def test_all_off_planes_give_zero_iou(dev):
    f = frame((8, 8), (20, 20), 9)
    f["left"][:] = -30.0
    f["right"][:] = -30.0
    counts, unions = run([f], thresholds(), dev)
    want_c, _ = reference(f, thresholds())
    assert np.array_equal(counts[0], want_c) and not unions[0].any()
    assert np.all(counts[0][:, 2] == 0) and np.all(counts[0][:, 0] == 0) and np.all(counts[0][:, 1] == counts[0][:, 3])
    assert counts[0][0, 3] > 0 and R.iou_iocm(counts[0][0]) == (0.0, 0.0)


@pytest.mark.parametrize("src_hw,dst_hw", [((9, 9), (9, 9)), ((9, 9), (20, 23))])
def test_logits_on_and_around_each_threshold(dev, src_hw, dst_hw):
    """Exactly on a threshold (off: the compare is strict), one ulp either side, -0.0 (not > 0.0), NaN (off at every threshold)."""
    ths = thresholds()
    f = frame(src_hw, dst_hw, 13)
    vals = []
    for th in ths:
        t = np.float32(th)
        vals += [t, np.nextafter(t, np.float32(np.inf)), np.nextafter(t, np.float32(-np.inf))]
    vals += [np.float32(-0.0), np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(1e-45)]
    flat = f["left"].reshape(-1)
    flat[:len(vals)] = vals
    f["right"][:] = -30.0
    f["right"][4, 4] = np.nan
    want_c, want_u = reference(f, ths)
    counts, unions = run([f], ths, dev)
    assert np.array_equal(unions[0], want_u) and np.array_equal(counts[0], want_c)
    if src_hw == dst_hw:      # the identity: the planted values read off directly
        on = unions[0].reshape(len(ths), -1)
        for k in range(len(ths)):
            assert (on[k, 3 * k], on[k, 3 * k + 1], on[k, 3 * k + 2]) == (0, 1, 0)
        assert not on[:, len(vals) - 4].any() and on[:, len(vals) - 3].all() and not on[:, len(vals) - 2].any()
        assert on[-1, len(vals) - 5] == 0 and on[-1, len(vals) - 1] == 1          # -0.0 and the smallest denormal against 0.0


def test_a_batch_equals_its_frames_alone(dev):
    ths = thresholds()
    frames = [frame((17, 13), (6, 5), 21, tax=(0.7, 0.1, 0.1, 0.1)), frame((66, 70), (131, 67), 22, obj=(True, True)),
              frame((5, 7), (13, 11), 23, tax=None, gt=(False, True))]
    counts, unions = run(frames, ths, dev)
    for k, f in enumerate(frames):
        want_c, want_u = reference(f, ths)
        alone_c, alone_u = run([f], ths, dev)
        assert np.array_equal(counts[k], alone_c[0]) and np.array_equal(unions[k], alone_u[0])
        assert np.array_equal(counts[k], want_c) and np.array_equal(unions[k], want_u)


def test_repeat_runs_are_bitwise_equal(dev):
    f, (want_c, _) = pair_case(len(PAIRS) - 1)            # 256 -> 855: 179 workgroups add into the frame's counters
    a_c, a_u = run([f, f], thresholds(), dev)
    b_c, b_u = run([f, f], thresholds(), dev)
    assert np.array_equal(a_c, b_c) and all(np.array_equal(x, y) for x, y in zip(a_u, b_u))
    assert np.array_equal(a_c[0], want_c) and np.array_equal(a_c[1], want_c)


def test_counts_are_zeroed_by_the_call(dev):
    from haff import ops, scoring
    f = frame((5, 7), (13, 11), 31)
    d = {k: (None if f[k] is None else torch.from_numpy(f[k]).to(dev)) for k in ("left", "right", "taxonomy", "gt_left", "gt_right")}
    d["target_hw"] = f["target_hw"]
    dirty = torch.full((1, 2, 4), 12345, dtype=torch.int32, device=dev)
    got = ops.score_masks(scoring.pack_frames([d]), [0.0, 0.5], dev, out_counts=dirty)
    assert got.data_ptr() == dirty.data_ptr() and np.array_equal(got.cpu().numpy()[0], reference(f, [0.0, 0.5])[0])


def test_refusals(dev):
    import haff
    lib = haff.load_library()
    got, big = R.score_refusals(lib)
    assert all(v == -1 for v in got.values()), {k: v for k, v in got.items() if v != -1}
    assert all(v == -2 for v in big.values()), big
    from haff import ops
    with pytest.raises(haff.HaffLibraryError):
        ops.score_masks(R.descriptor_table(hb=4097, gt=(0, 0), obj=(0, 0)), [0.0], dev)
    with pytest.raises(haff.HaffLibraryError):
        ops.score_masks(R.descriptor_table(), [0.0] * 9, dev)
