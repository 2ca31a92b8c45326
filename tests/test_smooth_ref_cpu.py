"""Mask smoothing (ActAffordance/scripts/utils/gaussian.py), host side: the identity the device filter rests on, checked on the CPU
restatement (tests/smooth_ref.py); the one-mistake-at-a-time variants of that restatement, each failing on an input built for it;
cvlite.gaussian_blur7_u8 and the smooth.py tool against the restatement; the flags of inference.py; the entry point's declaration
and host-side refusals. Nothing here computes on a GPU."""
import ctypes
import os
import re
import shutil
import sys

import numpy as np
import pytest
from PIL import Image

import haff
from haff import cvlite, inference, postprocess, smooth

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/smooth_ref.py
import smooth_ref as S   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(1, 1), (1, 9), (2, 3), (3, 5), (7, 7), (17, 33), (24, 40)]
TAUS = (0.5, 0.25, 0.9)
LO, HI = np.float32(-4.0), np.float32(3.0)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_quantile_then_threshold_is_threshold_then_blur(shape):
    """255 [quantile7(logit, need(tau)) > lt] == files_route(logit, lt, tau) at every pixel, for Gaussian, tie-heavy and NaN / inf
    planted planes, three tau and six logit thresholds; and the quantile is always one of the plane's own values (or -inf)."""
    rng = np.random.default_rng(shape[0] * 100 + shape[1])
    for name, x in S.fields(shape, rng):
        own = set(x[~np.isnan(x)].view(np.uint32).tolist()) | {np.float32(-np.inf).view(np.uint32).item()}
        for tau in TAUS:
            q = S.quantile7(x, S.need(tau))
            assert not np.isnan(q).any() and set((q + np.float32(0)).ravel().view(np.uint32).tolist()) <= own | {0}, (name, tau)
            for lt in S.LOGIT_THRESHOLDS:
                got = (q > np.float32(lt)).astype(np.uint8) * 255
                want = S.files_route(x, lt, tau)
                assert np.array_equal(got, want), (shape, name, tau, lt, int((got != want).sum()))


def test_need_values():
    assert [S.need(t) for t in (0.1, 0.25, 0.5, 0.75, 0.9)] == [6554, 16320, 32768, 49217, 58983]
    assert [postprocess.smooth_need(t) for t in (0.1, 0.25, 0.5, 0.75, 0.9)] == [6554, 16320, 32768, 49217, 58983]
    assert postprocess.smooth_need() == 32768
    for t in (0.0, 0.001, 1 / 255, 0.3333, 0.5019607843137255, 0.996, 0.9999):
        assert postprocess.smooth_need(t) == S.need(t) and 1 <= S.need(t) <= S.TOTAL, t
    for bad in (-0.01, 1.0, 1.5, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            postprocess.smooth_need(bad)
    # need is the first weight that survives: a plane of weight M blurs to (255 M + 32768) >> 16
    for t in (0.1, 0.25, 0.5, 0.75, 0.9):
        n = S.need(t)
        assert ((255 * n + 32768) >> 16) / 255.0 > t and not ((255 * (n - 1) + 32768) >> 16) / 255.0 > t


def _stripe(shape, axis, at, width):
    x = np.full(shape, LO, np.float32)
    if axis == "v":
        x[:, at:at + width] = HI
    else:
        x[at:at + width, :] = HI
    return x


def test_the_stripe_tie():
    """A 2-pixel stripe has weight (72 + 56) * 256 = 32768 on its own pixels, exactly need(0.5): it survives whole and grows by
    nothing ((56 + 28) * 256 beside it). A 1-pixel stripe (72 * 256) vanishes."""
    for axis in "vh":
        two, one = _stripe((20, 20), axis, 9, 2), _stripe((20, 20), axis, 9, 1)
        q2, q1 = S.quantile7(two, 32768), S.quantile7(one, 32768)
        assert np.array_equal(q2, two) and (q1 == LO).all()
        assert np.array_equal(S.files_route(two, 0.0), (two > 0).astype(np.uint8) * 255)
        assert not S.files_route(one, 0.0).any()


def test_variant_strict_compare_fails_at_the_tie():
    two = _stripe((20, 20), "v", 9, 2)
    wrong = S.smoothed_plane(two, 0.0, 32768, strict=True)
    assert not wrong.any() and S.files_route(two, 0.0).any()


def test_variant_border_reflect_fails_at_an_asymmetric_corner():
    """Column 0 and row 0 on, with the corner pixel off: under REFLECT_101 column -1 is column 1 (off), under REFLECT it is column 0
    (on), which lifts the border pixels from 72 * 256 to (72 + 56) * 256 = need."""
    x = np.full((12, 15), LO, np.float32)
    x[:, 0] = HI
    x[0, :] = HI
    x[0, 0] = LO
    right = S.smoothed_plane(x, 0.0, 32768)
    assert np.array_equal(right, S.files_route(x, 0.0))
    wrong = S.smoothed_plane(x, 0.0, 32768, border=S.reflect)
    assert not np.array_equal(wrong, right) and wrong[6, 0] == 255 and right[6, 0] == 0


def test_variant_transposed_weights_cannot_show_on_this_kernel():
    """The 7x7 table is the outer product of ONE vector with itself, so swapping the axes' weights changes nothing: no input can
    tell the two apart and this test does not pretend to. It shows the input WOULD tell them apart were the axes' tables different
    (an anisotropic pair of the same total), so that the equality below is a property of the kernel and not of a blind input."""
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((13, 22)) * 3).astype(np.float32)
    assert np.array_equal(S.quantile7(x, 32768, cy=S.COEFFS, cx=S.COEFFS[::-1]), S.quantile7(x, 32768))
    wide, narrow = (32, 36, 40, 40, 40, 36, 32), (0, 0, 64, 128, 64, 0, 0)
    assert sum(wide) == sum(narrow) == 256
    assert not np.array_equal(S.quantile7(x, 32768, cy=wide, cx=narrow), S.quantile7(x, 32768, cy=narrow, cx=wide))


def test_variant_nan_as_plus_inf_fails():
    """NaN taps are off in every `>` the consumers make. A plane that is mostly NaN is mostly off; counting NaN as +inf turns it on."""
    rng = np.random.default_rng(6)
    x = np.where(rng.random((16, 19)) < 0.7, np.float32(np.nan), LO).astype(np.float32)
    right = S.quantile7(x, 32768)
    assert not np.isnan(right).any() and np.array_equal(S.smoothed_plane(x, 0.0, 32768), S.files_route(x, 0.0))
    assert not S.files_route(x, 0.0).any()
    assert S.smoothed_plane(x, 0.0, 32768, nan_as=np.inf).any()
    # a pixel whose whole neighbourhood is NaN or -inf gets -inf
    y = np.full((9, 9), np.nan, np.float32)
    y[0, 0] = -np.inf
    assert (S.quantile7(y, 1) == -np.inf).all()
    y[4, 4] = 2.0
    q = S.quantile7(y, 72 * 72)
    assert q[4, 4] == 2.0 and (q[np.arange(9) != 4][:, np.arange(9) != 4] == -np.inf).all()


def test_variant_need_off_by_one_fails():
    """Every weight is a multiple of 64, so need(tau) - 1 is out of reach for the tabulated tau; the raw need is not. One hot pixel
    weighs 72 * 72 = 5184 at its own position: with need = 5185 the plane has weight exactly need - 1 there and the pixel goes."""
    x = np.full((9, 9), LO, np.float32)
    x[4, 4] = HI
    assert S.quantile7(x, 5184)[4, 4] == HI and (S.quantile7(x, 5185) == LO).all()
    assert S.smoothed_plane(x, 0.0, 5185 - 1).any() and not S.smoothed_plane(x, 0.0, 5185).any()


def test_reflection_with_overshoot():
    for n in (1, 2, 3, 5):
        p = np.arange(-3, n + 3)
        want = [0] * len(p) if n == 1 else [abs((v + (n - 1)) % (2 * n - 2) - (n - 1)) for v in p.tolist()]
        assert S.reflect101(p, n).tolist() == want
        assert cvlite._reflect101(p, n).tolist() == want
    assert S.reflect101(np.arange(-3, 6), 3).tolist() == [1, 2, 1, 0, 1, 2, 1, 0, 1]


@pytest.mark.parametrize("shape", [(1, 1), (1, 9), (2, 3), (5, 4), (31, 45), (64, 64)], ids=lambda s: "%dx%d" % s)
def test_cvlite_blur_equals_the_restatement(shape):
    rng = np.random.default_rng(shape[0] + 1000 * shape[1])
    for img in (rng.integers(0, 256, shape, dtype=np.uint8), (rng.random(shape) < 0.5).astype(np.uint8) * 255,
                np.full(shape, 255, np.uint8), np.zeros(shape, np.uint8)):
        got = cvlite.gaussian_blur7_u8(img)
        assert got.dtype == np.uint8 and np.array_equal(got, S.blur7(img))
    assert (cvlite.gaussian_blur7_u8(np.full(shape, 201, np.uint8)) == 201).all()      # the weights sum to 2^16 exactly
    with pytest.raises(ValueError):
        cvlite.gaussian_blur7_u8(np.zeros(shape + (3,), np.uint8))
    with pytest.raises(ValueError):
        cvlite.gaussian_blur7_u8(np.zeros(shape, np.float32))


def test_smooth_tool_on_a_small_tree(tmp_path, capsys):
    """smooth.py rewrites every image below --input_dir in place (by lower-cased suffix), grey-scale read, 0 / 255 written; other
    files stay; an unreadable image is reported and skipped."""
    rng = np.random.default_rng(9)
    tree = tmp_path / "vis0.5"
    planes = {
        "a/f1/aff_left.png": (rng.random((23, 31)) < 0.5).astype(np.uint8) * 255,
        "a/f1/aff_right.PNG": (rng.random((23, 31)) < 0.3).astype(np.uint8) * 255,
        "b/grey.bmp": rng.integers(0, 256, (9, 14), dtype=np.uint8),
        "b/deep/er/one.tif": np.full((1, 1), 255, np.uint8),
    }
    for rel, plane in planes.items():
        (tree / rel).parent.mkdir(parents=True, exist_ok=True)
        Image.fromarray(plane).save(tree / rel)
    rgb = rng.integers(0, 256, (8, 8, 3), dtype=np.uint8)
    Image.fromarray(rgb).save(tree / "b" / "colour.png")
    (tree / "b" / "notes.txt").write_text("left alone")
    (tree / "b" / "broken.png").write_bytes(b"not a png")
    for tau, args in ((0.5, []), (0.25, ["--threshold", "0.25"])):
        work = tmp_path / f"work{tau}"
        shutil.copytree(tree, work)
        assert smooth.main(["--input_dir", str(work)] + args) == len(planes) + 1
        assert f"Warning: Failed to load image {work / 'b' / 'broken.png'}" in capsys.readouterr().out
        for rel, plane in planes.items():
            got = np.asarray(Image.open(work / rel))
            want = (S.blur7(plane) / 255.0 > tau).astype(np.uint8) * 255
            assert got.dtype == np.uint8 and np.array_equal(got, want), (rel, tau)
        grey = np.asarray(Image.fromarray(rgb).convert("L"))
        assert np.array_equal(np.asarray(Image.open(work / "b" / "colour.png")), (S.blur7(grey) / 255.0 > tau).astype(np.uint8) * 255)
        assert (work / "b" / "notes.txt").read_text() == "left alone" and (work / "b" / "broken.png").read_bytes() == b"not a png"
    # on a 0 / 255 plane the tool is the files route of the identity
    x = (rng.standard_normal((23, 31)) * 3).astype(np.float32)
    plane = (x > 0).astype(np.uint8) * 255
    assert np.array_equal(smooth.smooth_plane(plane, 0.5), S.files_route(x, 0.0, 0.5))
    with pytest.raises(SystemExit):
        smooth.main([])


def test_inference_flags():
    base = ["--benchmark-dir", "b"]
    a = inference.parse_args(base)
    assert a.smooth_masks is False and a.smooth_threshold == 0.5
    a = inference.parse_args(base + ["--smooth_masks"])
    assert a.smooth_masks is True and a.smooth_threshold == 0.5
    a = inference.parse_args(base + ["--smooth_masks", "--smooth_threshold", "0.25", "--score_only", "--write_records", "r.pt"])
    assert a.smooth_masks and a.smooth_threshold == 0.25 and a.score_only
    with pytest.raises(SystemExit, match="modifies --smooth_masks"):
        inference.parse_args(base + ["--smooth_threshold", "0.5"])
    for bad in ("1.0", "-0.1", "nan"):
        with pytest.raises(SystemExit, match="smooth_threshold"):
            inference.parse_args(base + ["--smooth_masks", "--smooth_threshold", bad])


class _Ops:
    """ops.mask_quantile7 on the CPU restatement, counting its calls"""
    def __init__(self):
        self.calls = []

    def mask_quantile7(self, logits, need):
        import torch
        self.calls.append((tuple(logits.shape), need))
        return torch.from_numpy(np.stack([S.quantile7(p.numpy(), need) for p in logits]))


def test_smooth_mask_lists_keeps_the_structure(monkeypatch):
    """Both hands of a frame in one call, empty entries passed through as they are, frames of different sizes side by side."""
    import torch
    fake = _Ops()
    monkeypatch.setattr(postprocess, "ops", fake)
    g = torch.Generator().manual_seed(3)
    empty = torch.zeros((0, 9, 12))
    left = [torch.randn((1, 9, 12), generator=g), empty, torch.randn((1, 5, 7), generator=g), empty]
    right = [torch.randn((1, 9, 12), generator=g), torch.randn((1, 9, 12), generator=g), empty.new_zeros((0, 5, 7)), empty]
    out_l, out_r = postprocess.smooth_mask_lists(left, right, 0.25)
    assert fake.calls == [((2, 9, 12), 16320), ((1, 9, 12), 16320), ((1, 5, 7), 16320)]
    assert out_l[1] is left[1] and out_r[2] is right[2] and out_l[3] is left[3] and out_r[3] is right[3]
    for got, src in zip(out_l + out_r, left + right):
        assert got.shape == src.shape and got.dtype == torch.float32
        for k in range(src.shape[0]):
            assert np.array_equal(got[k].numpy(), S.quantile7(src[k].numpy(), 16320))
    assert left[0].data_ptr() != out_l[0].data_ptr()     # the inputs are not written


def test_entry_point_declared_and_refuses_on_the_host():
    text = open(os.path.join(ROOT, "include", "haff_hip.h")).read()
    assert re.search(r"^int haff_mask_quantile7\(const float\* logits, int n, int H, int W, int need,\s+float\* out, void\* stream\);",
                     text, flags=re.M)
    assert "haff_mask_quantile7" in haff.EXPORTED_SYMBOLS
    assert "mask_smooth.hip" in open(os.path.join(ROOT, "2handedafforder_amd", "csrc", "Makefile")).read()
    if not os.path.exists(haff.LIB_PATH):
        haff.build_library()
    lib = haff.load_library()
    buf = (ctypes.c_char * 4096)()
    p = (ctypes.addressof(buf) + 15) & ~15
    q = p + 2048
    f = lib.haff_mask_quantile7
    assert f(None, 1, 4, 4, 32768, q, None) == -1 and f(p, 1, 4, 4, 32768, None, None) == -1
    assert f(p + 2, 1, 4, 4, 32768, q, None) == -1 and f(p, 1, 4, 4, 32768, q + 1, None) == -1
    assert f(p, 1, 4, 4, 32768, p, None) == -1                                         # in place
    assert f(p, 0, 4, 4, 32768, q, None) == -1 and f(p, -1, 4, 4, 32768, q, None) == -1
    assert f(p, 1, 0, 4, 32768, q, None) == -1 and f(p, 1, 4, 0, 32768, q, None) == -1
    assert f(p, 1, 4, 4, 0, q, None) == -1 and f(p, 1, 4, 4, 65537, q, None) == -1 and f(p, 1, 4, 4, -5, q, None) == -1
    assert f(p, 1, 4097, 4, 32768, q, None) == -2 and f(p, 1, 4, 4097, 32768, q, None) == -2
    assert f(p, 1, 4097, 4, 0, q, None) == -1                                          # a bad argument comes first
