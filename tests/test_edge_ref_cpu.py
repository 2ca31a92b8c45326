"""The references and tolerances of tests/test_edge_kernels_gpu.py, checked where no GPU is needed: that tests/edge_ref.py states
what the issue's cases expect, that the resize tolerance is satisfiable by an fp32 evaluation of the formula and sharp enough to
catch the two usual mistakes, and that the one-rounding expectations of patchify_u8 are unambiguous."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/edge_ref.py
import edge_ref as E   # noqa: E402


@pytest.mark.parametrize("V", E.ARGMAX_V)
def test_argmax_rows_expect_what_the_rule_says(V):
    """torch.argmax on the CPU is the reference; spell out what it gives on the named rows, so the GPU test's expectation is the
    rule (first maximum, NaN above everything, first NaN first), not an accident of this torch build."""
    x, names = E.argmax_rows(V)
    assert x.stride(0) > V and bool(torch.isinf(x.as_strided((x.shape[0], x.stride(0)), (x.stride(0), 1))[:, V:]).all())
    ref = dict(zip(names, E.argmax(x).tolist()))
    assert all(0 <= i < V for i in ref.values())
    assert ref["all equal"] == 0 and ref["all -inf"] == 0 and ref["all NaN"] == 0
    assert ref["maximum at V - 1"] == V - 1
    assert ref["one NaN"] == V // 2
    assert ref["one NaN after +inf"] == 2 * V // 3
    assert ref["two NaNs"] == V // 2
    for name, first in (("tie in one thread's eight loads", 3), ("tie across waves", 5),
                        ("tie across waves, lower index in the later wave", 70), ("tie across trips", min(9, V - 8193)),
                        ("tie of the last entry", V // 2), ("two NaNs across waves and trips", 5 + 1024)):
        if name in ref:
            assert ref[name] == first, name
    if V >= 8193:
        assert "tie across trips" in ref and "tie across waves" in ref
    if V == 32003:
        assert len(names) == 14


def test_upscale_reference_is_the_module_chain():
    """edge_ref.upscale_mask (from the packed up1 rows) against torch's own modules run on the NCHW tensor in float64."""
    n, h, w = 2, 3, 5
    up1, ln_w, ln_b, w2, b2, hyper = (t.double() for t in E.upscale_inputs(n, h, w, 5))
    u = torch.zeros((n, 64, 2 * h, 2 * w), dtype=torch.float64)
    for dy in range(2):
        for dx in range(2):
            blk = up1.view(n, h, w, 4, 64)[:, :, :, dy * 2 + dx]              # [n, h, w, 64]
            u[:, :, dy::2, dx::2] = blk.permute(0, 3, 1, 2)
    ct2 = torch.nn.ConvTranspose2d(64, 32, 2, 2).double()
    with torch.no_grad():
        for dy in range(2):
            for dx in range(2):
                ct2.weight[:, :, dy, dx] = w2.view(64, 4, 32)[:, dy * 2 + dx]
        ct2.bias.copy_(b2)
        t = F.layer_norm(u.permute(0, 2, 3, 1), (64,), ln_w, ln_b, 1e-6).permute(0, 3, 1, 2)
        ref = torch.einsum("nc,nchw->nhw", hyper, F.gelu(ct2(F.gelu(t))))
    got = E.upscale_mask(up1, ln_w, ln_b, w2, b2, hyper, n, h, w)
    assert got.shape == (n, 4 * h, 4 * w)
    assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()


@pytest.mark.parametrize("case", E.RESIZE_CASES + (E.RESIZE_BIG,), ids=lambda c: f"{c[1]}-{c[2]}-{c[3]}")
def test_resize_bound_is_satisfiable(case):
    """An fp32 evaluation of the formula stays within the derived bound of the float64 reference on every case, and reads nothing
    outside the crop (which holds NaN)."""
    _, _, crop, out = case
    x = E.resize_source(case, 11)
    ref = E.resize_bilinear(x, crop, out)
    assert bool(torch.isfinite(ref).all())
    tol = E.resize_case_tol(x, crop)
    err = E.max_err(E.resize_fp32(x, crop, out), ref)
    assert err <= tol, (err, tol)
    assert tol <= 1e-3          # N(0, 1) samples: the bound stays three orders below the data


@pytest.mark.parametrize("case", E.RESIZE_CASES, ids=lambda c: f"{c[1]}-{c[2]}-{c[3]}")
def test_resize_bound_is_sharp(case):
    """The same evaluation without the half-pixel offset, and with the second tap clamped to the source instead of the crop, falls
    outside the bound wherever the mistake changes the arithmetic at all: the half-pixel offset whenever the scale is not 1 and the
    crop has more than one sample along that axis, the clamp whenever the crop is smaller than the source along an axis that is
    upsampled past its last sample (finite noise outside the crop, so it is the value that is wrong, not a NaN)."""
    _, (hs, ws), (hc, wc), (ho, wo) = case
    noise = E.rand((case[0], hs, ws), 12)
    x = E.resize_source(case, 11, outside=noise)
    ref = E.resize_bilinear(x, (hc, wc), (ho, wo))
    tol = E.resize_case_tol(x, (hc, wc))
    assert E.max_err(E.resize_fp32(x, (hc, wc), (ho, wo)), ref) <= tol
    shifted = any(c > 1 and c != o for c, o in ((hc, ho), (wc, wo)))
    err = E.max_err(E.resize_fp32(x, (hc, wc), (ho, wo), half_pixel=False), ref)
    assert (err > 100 * tol) if shifted else (err <= tol), (err, tol)
    # the last output's coordinate c/o * (o - 0.5) - 0.5 lies past c - 1 exactly when o > c
    overruns = (hc < hs and ho > hc) or (wc < ws and wo > wc)
    err = E.max_err(E.resize_fp32(x, (hc, wc), (ho, wo), clamp_to_crop=False), ref)
    assert (err > 100 * tol) if overruns else (err <= tol), (err, tol)


def test_resize_sharpness_cases_exist():
    """At least one case each in which the two planted mistakes show (otherwise the test above proves nothing)."""
    shifted = [c for c in E.RESIZE_CASES if any(a > 1 and a != b for a, b in zip(c[2], c[3]))]
    overruns = [c for c in E.RESIZE_CASES if (c[2][0] < c[1][0] and c[3][0] > c[2][0]) or (c[2][1] < c[1][1] and c[3][1] > c[2][1])]
    assert len(shifted) >= 4 and len(overruns) >= 2


def test_threshold_values_hold_every_edge():
    ths = (0.0, 0.4054651)
    for total in E.THRESHOLD_TOTALS:
        seen = torch.cat([E.threshold_values(total, ths, s) for s in range(24)])
        t = np.float32(ths[1])
        for v in (float(t), float(np.nextafter(t, np.float32(1))), float(np.nextafter(t, np.float32(-1))), 1e-45, -1e-45,
                  E.INF, -E.INF):
            assert bool((seen == torch.tensor(v, dtype=torch.float32)).any()), (total, v)
        assert bool(torch.isnan(seen).any())
        zeros = seen[seen == 0]
        assert bool(torch.signbit(zeros).any()) and not bool(torch.signbit(zeros).all())
    x = torch.tensor([0.0, -0.0, 1e-45, -1e-45, E.INF, -E.INF, E.NAN, float(np.nextafter(np.float32(0), np.float32(1)))])
    assert E.threshold(x, (0.0,), 255).tolist() == [[0, 0, 255, 0, 255, 0, 0, 255]]
    assert E.threshold(x, (0.0, -E.INF), 1).tolist()[1] == [1, 1, 1, 1, 1, 0, 0, 1]


def test_softmax_reference_at_its_edges():
    x = E.softmax_rows_input(12, 7, 3)
    ref = E.softmax_rows(x)
    assert torch.allclose(ref[[0, 1, 2, 3, 5]].sum(-1), torch.ones(5, dtype=torch.float64), atol=1e-12)
    assert 0 < ref[0, 3] < 1e-69 and abs(ref[0, 0].item() - 1 / 6) < 1e-15   # exp(-160) / 6: nothing at fp32's 1e-6
    assert ref[1, 0] == 1.0
    assert torch.equal(ref[2], torch.full((7,), 1 / 7, dtype=torch.float64))
    assert int(torch.isinf(x[3]).sum()) == 3 and bool((ref[3][torch.isinf(x[3])] == 0).all()) and ref[3, 6] > 0
    assert bool(torch.isnan(ref[4]).all())                                    # one +inf: the definition gives NaN for the row
    plain = torch.softmax(x.double(), -1)
    assert torch.equal(torch.isnan(plain), torch.isnan(ref))
    assert (torch.nan_to_num(plain) - torch.nan_to_num(ref)).abs().max().item() < 1e-15


def test_patchify_u8_roundings_are_unambiguous():
    """Only 256 x 3 values exist. For each, the fp32 evaluation (subtract and divide, each correctly rounded: relative error at most
    (1 + U32)^2 - 1 < 2.0001 * U32, and one ulp is at least U32 * |v|... so within 2 ulp) is within 2 ulp of the float64 value, and
    rounding the fp32 value once more to bf16 / f16 gives the same as rounding the float64 value directly: "rounded once" does not
    depend on which of the two is meant."""
    raw = torch.arange(256, dtype=torch.uint8).view(1, 256, 1, 1).expand(1, 256, 1, 3).contiguous()     # one 256 x 1 frame
    ref = E.patchify_u8(raw, 1, 256, 1, 3, E.SAM_MEAN, E.SAM_STD)                                        # [256, 3] (P = 1)
    m, s = (torch.tensor(np.asarray(v, np.float32)) for v in (E.SAM_MEAN, E.SAM_STD))
    f32 = (torch.arange(256, dtype=torch.float32)[:, None] - m[None, :]) / s[None, :]
    assert bool(((f32.double() - ref).abs() <= 2 * E.ulp32(ref)).all())
    for dt in (torch.bfloat16, torch.float16):
        assert torch.equal(f32.to(dt), ref.to(dt))


def test_gather_references_agree_with_convolutions():
    """patchify rows times a flattened kernel are conv(k = s = P); im2col rows times a (ky, kx, c) kernel are conv 3x3 pad 1."""
    x = E.rand((2, 3, 50, 83), 1).double()
    w = E.rand((4, 3, 16, 16), 2).double()
    rows = E.patchify_nchw(x.float(), 16, 3, 5, 768, torch.float32).double()
    ref = F.conv2d(x.float().double()[:, :, :48, :80], w, stride=16).permute(0, 2, 3, 1).reshape(-1, 4)
    assert (rows @ w.reshape(4, -1).T - ref).abs().max().item() < 1e-10
    assert E.patchify_nchw(x.float(), 14, 2, 3, 592, torch.bfloat16)[:, 588:].abs().max().item() == 0
    xi = E.rand((2, 6, 7, 16), 3)
    wi = E.rand((8, 16, 3, 3), 4).double()
    cols = E.im2col3x3(xi).double()
    ref = F.conv2d(xi.double().permute(0, 3, 1, 2), wi, padding=1).permute(0, 2, 3, 1).reshape(-1, 8)
    assert (cols @ wi.permute(0, 2, 3, 1).reshape(8, -1).T - ref).abs().max().item() < 1e-10
    assert torch.equal(E.im2col3x3(xi, via=torch.float32), E.im2col3x3(xi))


def test_rope_reference_is_a_rotation():
    B, Tq, Hq, Hkv, d, Tmax = 2, 3, 4, 2, 16, 8
    cs = E.rope_table(Tmax, d)
    qkv = E.rand((B * Tq, (Hq + 2 * Hkv) * d + 8), 5)
    q, k, v = E.rope_cache(qkv, cs, B, Tq, Hq, Hkv, d, [0, Tmax - Tq])
    x = qkv.double()[:, :(Hq + 2 * Hkv) * d].reshape(B, Tq, Hq + 2 * Hkv, d)
    assert torch.equal(q[0, 0], x[0, 0, :Hq]) and torch.equal(k[0, 0], x[0, 0, Hq:Hq + Hkv])       # position 0: identity
    assert torch.equal(v, x[:, :, Hq + Hkv:])
    pair = lambda t: t[..., :d // 2] ** 2 + t[..., d // 2:] ** 2                                     # noqa: E731
    assert (pair(q) - pair(x[:, :, :Hq])).abs().max().item() < 1e-6                                  # norms of the rotated pairs
    # pair j of row (b=1, t=2) turns by the angle (Tmax - Tq + 2) * 10000^(-2j/d)
    j, pos = 3, Tmax - Tq + 2
    ang = pos * 10000.0 ** (-2.0 * j / d)
    x1, x2 = x[1, 2, 0, j].item(), x[1, 2, 0, j + d // 2].item()
    assert abs(q[1, 2, 0, j].item() - (x1 * np.cos(ang) - x2 * np.sin(ang))) < 1e-6
    assert abs(q[1, 2, 0, j + d // 2].item() - (x2 * np.cos(ang) + x1 * np.sin(ang))) < 1e-6
