"""The references, cases and bounds of tests/test_norm_ingest_kernels_gpu.py, checked where no GPU is needed: the restatements of
tests/norm_ingest_ref.py against independent references (torch's layer_norm, the RMS formula, Pillow, CLIPImageProcessor), the
fp32 evaluations inside their own bounds on every case, every deliberate mistake outside them, and the finalize arithmetic with
an fp32 and with a double 1 / C."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import norm_ingest_ref as N   # noqa: E402
import train_edge_ref as R   # noqa: E402

F32, F64, BF16, F16 = N.F32, N.F64, N.BF16, N.F16
SMALL_CASES = tuple(c for c in N.NORM_CASES if c[0] <= 5)


def _tables():
    import haff  # noqa: F401
    from haff.preprocess import pil_resample_tables
    return pil_resample_tables


# ------------------------------------------------------------------------------------------------- the case lists themselves
def test_cases_cover_what_the_dispatch_rule_distinguishes():
    assert {c for _, c in N.NORM_CASES} == set(N.NORM_C) and {r for r, _ in N.NORM_CASES} == set(N.NORM_ROWS)
    by_c = {}
    for rows, C in N.NORM_CASES:
        by_c.setdefault(C, set()).add(N.selected_kernel(rows, C))
    for C in N.NORM_C:
        assert by_c[C] == ({"wg", "wave"} if 2048 <= C <= 6144 else {"wave"}), C
    # the four corners of the rule, and a map at a workgroup-kernel width
    assert N.selected_kernel(256, 2048) == "wg" and N.selected_kernel(257, 2048) == "wave"
    assert N.selected_kernel(256, 2040) == "wave" and N.selected_kernel(256, 6144) == "wg" and N.selected_kernel(256, 6152) == "wave"
    assert N.selected_kernel(5, 4096, mapped=True) == "wave"
    # every instantiated arm, three of them entered below their width
    assert {N.nch_arm(C) for C in N.NORM_C} == {1, 2, 3, 4, 8, 10, 16}
    assert (N.nch_arm(2568), N.nch_arm(4104), N.nch_arm(5128)) == (8, 10, 16) and -(-5128 // 512) == 11
    assert all(C % 8 == 0 and C <= N.C_MAX for C in N.NORM_C)
    for axis, (B, (Hi, Wi), (Ho, Wo)) in N.OVER_CAP.items():
        units = B * Ho * Wo * (1 if axis == 0 else 3)
        assert N.GRID_CAP < units < N.GRID_CAP + 65536 and (units - N.GRID_CAP) % 256 != 0
        assert (Hi == Ho) if axis == 0 else (Wi == Wo)
    B, _, _, _, S = N.CLIP_OVER_CAP
    assert N.GRID_CAP < B * 3 * S * S < N.GRID_CAP + 65536


def test_row_sum_orders_add_every_column_once():
    """integers sum exactly in any order: both orders equal the plain sum at every C, partly filled chunks included"""
    for C in N.NORM_C:
        v = torch.arange(3 * C, dtype=F32).reshape(3, C) % 251
        for kernel in ("wave", "wg"):
            assert torch.equal(N.row_sum(v, kernel), v.sum(-1)), (C, kernel)
    assert N.chain(4096, "wave") == 70 and N.chain(4096, "wg") == 24 and N.chain(8, "wave") == 14


# ------------------------------------------------------------------------------------------- restatements vs independent ones
@pytest.mark.parametrize("rows,C", SMALL_CASES + ((256, 2048),))
def test_norm_restatements_equal_torch(rows, C):
    x = N.norm_inputs(rows, C, C + rows, F32)
    w, b = N.norm_weights(C, C)
    ref = F.layer_norm(x.double(), (C,), w.double(), b.double(), N.f32(N.EPS_LN))
    got = N.norm(x, w, b, False, N.EPS_LN)
    assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()
    xd = x.double()
    rms = xd * torch.rsqrt(xd.pow(2).mean(-1, keepdim=True) + N.f32(N.EPS_RMS)) * w.double()
    assert (N.norm(x, w, None, True, N.EPS_RMS) - rms).abs().max().item() <= 1e-12 * rms.abs().max().item()
    mean, rstd = N.row_stats(x, False, N.EPS_LN)
    assert torch.allclose(mean, xd.mean(-1), rtol=1e-13, atol=1e-15)
    assert torch.allclose(rstd, 1.0 / torch.sqrt(xd.var(-1, unbiased=False) + N.f32(N.EPS_LN)), rtol=1e-12, atol=0)
    m0, r0 = N.row_stats(x, True, N.EPS_RMS)
    assert bool((m0 == 0).all()) and torch.allclose(r0, torch.rsqrt(xd.pow(2).mean(-1) + N.f32(N.EPS_RMS)), rtol=1e-12, atol=0)


def test_gather_restatement():
    y = torch.arange(12.0).reshape(4, 3) + 1
    for name in N.MAP_CASES:
        m = N.gather_map(name, 4)
        out = N.gather(y, m)
        assert out.shape == (len(m), 3) and (len(m) % 4 != 0 or name in ("all -1", "permutation"))
        for i, src in enumerate(m.tolist()):
            assert torch.equal(out[i], y[src] if src >= 0 else torch.zeros(3))
            assert src < 4
    assert bool((N.gather_map("all -1", 4) == -1).all()) and len(N.gather_map("longer than the input", 4)) > 4
    assert len(set(N.gather_map("duplicates", 4).tolist())) < 5


# ------------------------------------------------------------------------------------------------------ bounds that hold
def _codes():
    return [(code, rms) for code in N.NORM_CODES for rms in (False, True)]


@pytest.mark.parametrize("code,rms", _codes(), ids=lambda v: ("rms" if v else "ln") if isinstance(v, bool) else N.CODE_IDS[v])
def test_fp32_evaluation_stays_within_the_bound(code, rms):
    """On every shape case (the small-row ones and both kernels at 2048) and every named value row: the fp32 evaluation in the
    OTHER kernel's order, rounded to the storage type, is inside the bound built from the selected kernel's order."""
    tin, tout = N.NORM_CODES[code]
    eps = N.EPS_RMS if rms else N.EPS_LN
    for rows, C in SMALL_CASES + ((256, 2048), (257, 2048)):
        x = N.norm_inputs(rows, C, C + rows, tin)
        w, b = N.norm_weights(C, C)
        b = None if rms else b
        for kernel in ("wave", "wg"):
            ref, bnd = N.expect_norm(x, w, b, rms, eps, tout, kernel)
            other = N.norm(x, w, b, rms, eps, F32, "wg" if kernel == "wave" else "wave").to(tout)
            assert R.ratio(other, ref, bnd) <= 1.0, (rows, C, kernel)
    for C in N.VALUE_C:
        x, names = N.value_rows(C, C, tin, rms)
        w, b = N.norm_weights(C, C)
        b = None if rms else b
        for kernel in ("wave", "wg"):
            ref, bnd = N.expect_norm(x, w, b, rms, eps, tout, kernel)
            other = N.norm(x, w, b, rms, eps, F32, "wg" if kernel == "wave" else "wave").to(tout)
            for i, name in enumerate(names):
                assert R.ratio(other[i], ref[i], bnd[i]) <= 1.0, (C, kernel, name)
            # the bad rows are bad where the reference is, and nowhere else
            nan_row, inf_row = names.index("one NaN"), names.index("one +inf")
            assert bool(torch.isnan(ref[nan_row]).all())
            if rms:
                bad = torch.zeros(C, dtype=torch.bool)
                bad[2 * C // 3] = True
                assert torch.equal(torch.isnan(ref[inf_row]), bad) and bool((ref[inf_row][~bad] == 0).all())
            else:
                assert bool(torch.isnan(ref[inf_row]).all())
            good = [i for i, n in enumerate(names) if n not in ("one NaN", "one +inf")]
            assert bool(torch.isfinite(ref[good]).all())


@pytest.mark.parametrize("dtype", (F32, BF16, F16), ids=lambda d: R.IDS[d])
@pytest.mark.parametrize("rms", (False, True), ids=("ln", "rms"))
def test_fp32_statistics_stay_within_the_bound(rms, dtype):
    eps = N.EPS_RMS if rms else N.EPS_LN
    xs = [N.norm_inputs(rows, C, C + rows, dtype) for rows, C in SMALL_CASES]
    xs += [N.value_rows(C, C, dtype, rms)[0] for C in N.VALUE_C]
    for x in xs:
        (m, bm), (r, br) = N.expect_stats(x, rms, eps)
        # a plain left-to-right fp32 sum: a third order, neither kernel's
        xf = x.float()
        if rms:
            m32, r32 = torch.zeros(x.shape[0]), 1.0 / torch.sqrt(R.seq_sum32(xf * xf, 1) / x.shape[1] + N.f32(eps))
        else:
            m32 = R.seq_sum32(xf, 1) / x.shape[1]
            r32 = 1.0 / torch.sqrt(R.seq_sum32((xf - m32[:, None]) ** 2, 1) / x.shape[1] + N.f32(eps))
        # a left-to-right sum has a chain of C additions, not chain(C): only the rows it adds exactly, or nearly, are held to it
        if x.shape[1] <= 72:
            assert R.ratio(m32, m, bm * (x.shape[1] / N.chain(x.shape[1], "wave"))) <= 1.0
            assert R.ratio(r32, r, br * (x.shape[1] / N.chain(x.shape[1], "wave"))) <= 1.0
        m_k, r_k = N.row_stats(x, rms, eps, F32, "wave")
        assert R.ratio(m_k, m, bm) <= 0.25 + 1e-9 and R.ratio(r_k, r, br) <= 0.25 + 1e-9      # K = 4 times its own error, at least


def test_constant_row_is_why_the_conditioning_term_exists():
    """fp32 gets the row of 3.0 exactly right and the row of 0.1 wrong by d mean * rstd; the conditioning term covers the second
    whichever way the additions are ordered, and is small: well under one part in 1e3 of an ordinary row's output."""
    C = 1280
    x, names = N.value_rows(C, C, F32, False)
    w, b = N.norm_weights(C, C)
    ref = N.norm(x, w, b, False, N.EPS_LN)
    i3, i01, i0 = names.index("constant 3"), names.index("constant 0.1"), names.index("ordinary")
    for kernel in ("wave", "wg"):
        ev = N.norm(x, w, b, False, N.EPS_LN, F32, kernel)
        assert torch.equal(ev[i3].double(), b.double()) and torch.equal(ref[i3], b.double())
        cond = N.cond_terms(x, w, False, N.EPS_LN, kernel)[0]
        assert ((ev[i01].double() - ref[i01]).abs() <= cond[i01] + 2 * N.U32 * b.abs().double()).all()
        assert cond[i0].max().item() <= 1e-4 * ref[i0].abs().max().item()


# ------------------------------------------------------------------------------------------------------ bounds that bite
@pytest.mark.parametrize("wrong", N.WRONG_NORM, ids=lambda d: next(iter(d)))
def test_every_wrong_variant_misses_the_bound(wrong):
    """on at least one case, each named: the shape cases and the value rows, in fp32 storage (a 16-bit output hides 2^-9)"""
    rms = "rms_centred" in wrong
    misses = []
    for rms_case in ((True,) if rms else (False, True)):
        eps = N.EPS_RMS if rms_case else N.EPS_LN
        for rows, C in SMALL_CASES:
            x = N.norm_inputs(rows, C, C + rows, F32)
            w, b = N.norm_weights(C, C)
            ref, bnd, bad = N.expect_norm(x, w, None if rms_case else b, rms_case, eps, F32, "wave", **wrong)
            if R.ratio(bad, ref, bnd) > 1.0:
                misses.append(("y", rms_case, rows, C))
            (m, bm), (r, br), (m_bad, r_bad) = N.expect_stats(x, rms_case, eps, **wrong)
            if R.ratio(m_bad, m, bm) > 1.0 or R.ratio(r_bad, r, br) > 1.0:
                misses.append(("stats", rms_case, rows, C))
    print(next(iter(wrong)), "missed on", misses)
    assert any(m[0] == "y" for m in misses) and any(m[0] == "stats" for m in misses)
    if "drop_last_8" in wrong or "round_c_to_64" in wrong:
        # the mistakes a partly filled chunk provokes are caught AT the partly filled widths, and at the widest row
        hit = {m[3] for m in misses if m[0] == "y"}
        assert {72, 520} <= hit and (8192 in hit or "round_c_to_64" in wrong), hit


def test_a_lost_chunk_is_caught_at_4096_in_every_storage_type():
    """8 columns of 4096 dropped barely move the statistics; the outputs there are wrong by their own size"""
    C = 4096
    for code, (tin, tout) in N.NORM_CODES.items():
        x = N.norm_inputs(3, C, 7, tin)
        w, b = N.norm_weights(C, C)
        ref, bnd, bad = N.expect_norm(x, w, b, False, N.EPS_LN, tout, "wg", drop_last_8=True)
        assert R.ratio(bad.to(tout), ref, bnd) > 1.0, code


# ---------------------------------------------------------------------------------------------------------------- finalize
@pytest.mark.parametrize("slots", N.FINALIZE_SLOTS)
@pytest.mark.parametrize("rows", N.FINALIZE_ROWS)
def test_finalize_in_double_meets_the_tight_bound(rows, slots):
    C = 64 * slots
    part, names = N.finalize_partials(rows, slots)
    mean, rstd, ratio = N.finalize_exact(part, C, N.FINALIZE_EPS)
    bm, br = N.finalize_bounds(mean, rstd, C, N.FINALIZE_EPS)
    gm, gr = N.finalize(part, C, N.FINALIZE_EPS)
    assert (np.abs(gm - mean) <= bm).all() and (np.abs(gr - rstd) <= br).all()
    for r, name in enumerate(names):
        if name.startswith("ratio"):
            want = float(name.split()[1])
            assert want <= ratio[r] <= want + 7 and abs(rstd[r] - 1 / np.sqrt(1 + N.f32(N.FINALIZE_EPS))) < 1e-15
        if name in ("negative", "zero"):
            assert ratio[r] == N.INF or mean[r] == 0
            assert rstd[r] == 1 / np.sqrt(N.f32(N.FINALIZE_EPS))
    if rows >= 255:
        assert set(names) == set(N.FINALIZE_PATTERNS)
        # the clamp is exercised: without it the variance of a "negative" row is below zero
        r = names.index("negative")
        s = part[r].astype(np.float64).sum(0)
        assert s[1] / C - (s[0] / C) ** 2 < 0


def test_finalize_with_an_fp32_reciprocal_misses_the_tight_bound_at_1280():
    """1 / 1280 rounded to fp32 is off by 1.5e-8 relative; the variance then carries -e mean^2: 7.5e-5 of rstd at mean / std = 100
    and 7.5e-3 at 1000, against a bound of 2.4e-7. The same arithmetic with the division in double meets it."""
    C, slots = 1280, 20
    e = float(np.float32(1.0) / np.float32(C)) * C - 1.0
    assert 1.4e-8 < abs(e) < 1.6e-8
    part, names = N.finalize_partials(257, slots)
    mean, rstd, ratio = N.finalize_exact(part, C, N.FINALIZE_EPS)
    bm, br = N.finalize_bounds(mean, rstd, C, N.FINALIZE_EPS)
    gm, gr = N.finalize(part, C, N.FINALIZE_EPS, inv_c_fp32=True)
    for want, rel in (("ratio 100", 7.5e-5), ("ratio 1000", 7.5e-3)):
        idx = [r for r, n in enumerate(names) if n == want]
        err = np.abs(gr[idx] - rstd[idx]) / rstd[idx]
        assert (err > 100 * br[idx] / rstd[idx]).all() and (0.5 * rel < err).all() and (err < 2.1 * rel).all(), (want, err.max())
    gm, gr = N.finalize(part, C, N.FINALIZE_EPS)
    assert (np.abs(gm - mean) <= bm).all() and (np.abs(gr - rstd) <= br).all()
    assert (br / rstd < 3e-7).all()


# ------------------------------------------------------------------------------------------------------------ frame ingest
@pytest.mark.parametrize("filt", N.FILTERS)
@pytest.mark.parametrize("geom", N.GEOMETRIES, ids=lambda g: f"{g[0][0]}x{g[0][1]}-{g[1][0]}x{g[1][1]}")
def test_resample_restatement_equals_pillow(geom, filt):
    from PIL import Image
    tables = _tables()
    (H, W), out = geom
    pil = Image.BILINEAR if filt == "bilinear" else Image.BICUBIC
    clipped_low = clipped_high = False
    for kind in N.IMAGE_KINDS:
        img = N.image(kind, 2, H, W, seed=H + W)
        got = N.resize(img, out, filt, tables)
        assert got.shape == (2, out[0], out[1], 3) and got.dtype == np.uint8
        for b in range(2):
            ref = np.asarray(Image.fromarray(img[b]).resize((out[1], out[0]), pil))
            assert np.array_equal(got[b], ref), (kind, b)
        if kind == "all 255":
            assert bool((got == 255).all())
        if kind == "all 0":
            assert bool((got == 0).all())


def test_checkerboard_makes_both_clips_run():
    """bicubic on the 0 / 255 checkerboard: before the clamp the accumulator goes below 0 and above 255"""
    tables = _tables()
    bounds, coeffs = tables(9, 23, "bicubic")
    row = N.image("checkerboard", 1, 1, 9)[0, 0, :, 0].astype(np.int64)
    acc = np.array([(1 << 21) + int((coeffs[o, :bounds[o, 1]] * row[bounds[o, 0]:bounds[o, 0] + bounds[o, 1]]).sum()) for o in range(23)]) >> 22
    assert acc.min() < 0 and acc.max() > 255


def test_over_cap_shapes_are_within_the_restatement():
    """the tables of the two over-cap shapes are in range and the restatement runs them (its own overflow assertion included)"""
    tables = _tables()
    for axis, (B, (Hi, Wi), (Ho, Wo)) in N.OVER_CAP.items():
        n_in, n_out = (Wi, Wo) if axis == 0 else (Hi, Ho)
        bounds, coeffs = tables(n_in, n_out, "bicubic")
        assert int((bounds[:, 0] + bounds[:, 1]).max()) <= n_in and int(bounds[:, 0].min()) >= 0
        out = N.resample_axis(N.image("checkerboard", 1, Hi if axis == 0 else Hi, 7 if axis == 1 else Wi), axis, bounds, coeffs)
        assert out.shape[1:3] == ((Hi, Wo) if axis == 0 else (Ho, 7))


@pytest.mark.parametrize("hw", [(300, 400), (97, 131), (224, 224)])
def test_clip_restatement_matches_clip_image_processor(hw):
    tr = pytest.importorskip("transformers")
    import haff  # noqa: F401
    from haff import preprocess as P
    img = N.image("random", 1, hw[0], hw[1], seed=5)
    nh, nw = P.clip_resize_shape(hw[0], hw[1], 224)
    x = N.resize(img, (nh, nw), "bicubic", P.pil_resample_tables)
    got = N.clip_normalize(x, (nh - 224) // 2, (nw - 224) // 2, 224, P.clip_normalize_lut())
    ref = tr.CLIPImageProcessor().preprocess(img[0], return_tensors="pt")["pixel_values"][0].numpy()
    assert got.shape == (1, 3, 224, 224) and np.abs(got[0] - ref).max() <= 1e-6


def test_clip_cases_and_every_byte_frame():
    for B, (H, W), top, left, S in N.CLIP_CASES + (N.CLIP_OVER_CAP,):
        assert 0 <= top and top + S <= H and 0 <= left and left + S <= W
    cases = N.CLIP_CASES
    assert any(S == 1 for *_, S in cases) and any((H, W) == (S, S) for _, (H, W), _, _, S in cases)
    assert any(top != (H - S) // 2 or left != (W - S) // 2 for _, (H, W), top, left, S in cases) and any(H != W for _, (H, W), *_ in cases)
    f = N.every_byte_frame(2, 16, 16)
    for b in range(2):
        for c in range(3):
            assert len(np.unique(f[b, :, :, c])) == 256
    lut = np.arange(768, dtype=np.float32).reshape(3, 256)
    out = N.clip_normalize(f, 0, 0, 16, lut)
    assert sorted(out.reshape(2, 3, -1)[1, 2].tolist()) == list(range(512, 768))
