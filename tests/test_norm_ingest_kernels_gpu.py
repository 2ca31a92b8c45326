"""The kernels of csrc/norm.hip and csrc/frame_ingest.hip at their edges, each called through its C entry point and compared on the
CPU with the restatements of tests/norm_ingest_ref.py (checked on their own by tests/test_norm_ingest_ref_cpu.py).

Norms and row statistics: float64 reference, bound = train_edge_ref.bound (4 x the error of the fp32 evaluation in the selected
kernel's order + 8 fp32 ulps of the row's scale + half an ulp of the storage type) + the derived conditioning terms
(norm_ingest_ref.cond_terms). Finalize: exact rational reference from exact partials, 2 fp32 ulps. Resampling and the CLIP lookup:
array_equal / torch.equal. Every output buffer is a row longer and, where the entry point takes a row stride, wider than the
kernel's share, and pre-filled with a sentinel that has to survive; the padding columns of x hold NaN. Each comparison prints its
ratio to the bound; the module prints the worst per entry point at the end."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_ref as E   # noqa: E402
import norm_ingest_ref as N   # noqa: E402
import train_edge_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu

BAD_ARG, UNSUPPORTED = -1, -2
F32, F64, BF16, F16 = R.F32, R.F64, R.BF16, R.F16
WORST = {}
KERNELS = {}          # entry point -> the kernels the dispatch rule selected for the cases that ran
_case_id = lambda c: f"{c[0]}x{c[1]}"   # noqa: E731
_code_id = lambda c: N.CODE_IDS[c]   # noqa: E731


def _lib():
    import haff  # noqa: F401
    from haff.lib import load_library
    return load_library()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


def _check(name, got, ref, bnd, what=""):
    r = R.ratio(got, ref, bnd)
    WORST[name] = max(WORST.get(name, 0.0), r)
    print(f"{name} {what}: ratio to bound {r:.3g}")
    assert r <= 1.0, f"{name} {what}: |err| / bound = {r:.3g}"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for name in sorted(WORST):
        print(f"WORST {name}: {WORST[name]:.3g}")
    for name in sorted(KERNELS):
        print(f"KERNELS {name}: {sorted(KERNELS[name])}")


def _out(rows, ld, dtype, dev):
    """a sentinel-filled [rows + 1, ld] output"""
    return torch.full((rows + 1, ld), R.SENT, dtype=dtype, device=dev)


def _share(y, rows, C, what):
    """the kernel's [rows, C] share on the CPU, after checking that the padding columns and the row after the last kept the sentinel"""
    full = y.cpu()
    assert bool((full[:rows, C:] == R.SENT).all()), f"{what}: padding columns of y written"
    assert bool((full[rows:] == R.SENT).all()), f"{what}: the row after the last written"
    return full[:rows, :C].contiguous()


def _norm_call(lib, rms, xg, ldx, y, ldy, wg, bg, mg, rows, C, eps, code):
    if rms:
        return lib.haff_rmsnorm(_p(xg), ldx, _p(y), ldy, _p(wg), rows, C, eps, code, _s())
    return lib.haff_layernorm(_p(xg), ldx, _p(y), ldy, _p(wg), _p(bg), _p(mg), rows, C, eps, code, _s())


def _run_norm(dev, rms, x, w, b, code, in_map=None, pads=((0, 0), (8, 16))):
    """-> [y [rows_out, C] on the CPU for each (x padding, y padding)]; x's padding holds NaN, y's the sentinel"""
    lib = _lib()
    tout = N.NORM_CODES[code][1]
    C = x.shape[1]
    rows = x.shape[0] if in_map is None else len(in_map)
    eps = N.EPS_RMS if rms else N.EPS_LN
    wg, bg = w.to(dev), (None if rms else b.to(dev))
    mg = None if in_map is None else in_map.to(dev)
    outs = []
    for px, py in pads:
        xg = E.widen(x, px, R.NAN).to(dev)
        y = _out(rows, C + py, tout, dev)
        assert _norm_call(lib, rms, xg, C + px, y, C + py, wg, bg, mg, rows, C, eps, code) == 0
        outs.append(_share(y, rows, C, f"ldx {C + px} ldy {C + py}"))
    return outs


# ------------------------------------------------------------------------------------------------ haff_layernorm / haff_rmsnorm
@pytest.mark.parametrize("code", N.NORM_CODES, ids=_code_id)
@pytest.mark.parametrize("case", N.NORM_CASES, ids=_case_id)
def test_norm_shapes(dev, case, code):
    """Every row length and row count of the case list, LayerNorm and RMSNorm, ld == C and ld > C (NaN right of x's C columns, the
    sentinel right of y's and in the row after the last); the bound is built in the order of the kernel the dispatch rule selects."""
    rows, C = case
    tin, tout = N.NORM_CODES[code]
    kernel = N.selected_kernel(rows, C)
    x = N.norm_inputs(rows, C, C + rows, tin)
    w, b = N.norm_weights(C, C)
    for rms in (False, True):
        name = "rmsnorm" if rms else "layernorm"
        KERNELS.setdefault(name, set()).add(kernel)
        ref, bnd = N.expect_norm(x, w, None if rms else b, rms, N.EPS_RMS if rms else N.EPS_LN, tout, kernel)
        tight, wide = _run_norm(dev, rms, x, w, b, code)
        _check(name, tight, ref, bnd, f"{rows}x{C} {kernel} {N.CODE_IDS[code]} ld == C")
        _check(name, wide, ref, bnd, f"{rows}x{C} {kernel} {N.CODE_IDS[code]} ld > C")
        assert torch.equal(tight, wide), "the row strides change the result"


def test_norm_shapes_met_both_kernels():
    """the case list reaches the wave-per-row and the workgroup-per-row kernel (the latter only where both exist)"""
    seen = {N.selected_kernel(r, c) for r, c in N.NORM_CASES}
    assert seen == {"wave", "wg"}
    for C in N.NORM_C:
        both = {N.selected_kernel(r, c) for r, c in N.NORM_CASES if c == C}
        assert both == ({"wave", "wg"} if 2048 <= C <= 6144 else {"wave"}), C


@pytest.mark.parametrize("code", N.NORM_CODES, ids=_code_id)
@pytest.mark.parametrize("rms", [False, True], ids=["ln", "rms"])
def test_norm_value_rows(dev, rms, code):
    """The named rows at C = 72, 1280 and 4096 (there through both kernels: alone, and with an identity map, which selects the
    wave-per-row kernel): each row within its own bound, the NaN / +inf rows non-finite exactly where the reference is."""
    tin, tout = N.NORM_CODES[code]
    name = "rmsnorm" if rms else "layernorm"
    eps = N.EPS_RMS if rms else N.EPS_LN
    for C in N.VALUE_C:
        x, names = N.value_rows(C, C, tin, rms)
        w, b = N.norm_weights(C, C)
        runs = [(None, N.selected_kernel(len(names), C))]
        if C == 4096 and not rms:
            runs.append((torch.arange(len(names), dtype=torch.int32), "wave"))
        for in_map, kernel in runs:
            ref, bnd = N.expect_norm(x, w, None if rms else b, rms, eps, tout, kernel)
            for got in _run_norm(dev, rms, x, w, b, code, in_map):
                for i, row in enumerate(names):
                    _check(f"{name} values", got[i], ref[i], bnd[i], f"C {C} {kernel} {N.CODE_IDS[code]} row '{row}'")


@pytest.mark.parametrize("code", N.NORM_CODES, ids=_code_id)
def test_layernorm_gather_map(dev, code):
    """in_map: all -1, duplicates, longer than the input, a permutation; output row counts 4, 5, 13 (not multiples of 4). At 2048
    and 4096 the unmapped call would take the workgroup kernel, which has no map: a mapped call must still gather. Dropped rows are
    +0 in every bit."""
    tin, tout = N.NORM_CODES[code]
    for C in (72, 2048, 4096):
        x = N.norm_inputs(5, C, C, tin)
        w, b = N.norm_weights(C, C)
        ref, bnd = N.expect_norm(x, w, b, False, N.EPS_LN, tout, "wave")
        for mname in N.MAP_CASES:
            m = N.gather_map(mname, 5)
            for got in _run_norm(dev, False, x, w, b, code, m):
                _check("layernorm map", got, N.gather(ref, m), N.gather(bnd, m) + 1e-300, f"C {C} '{mname}' {N.CODE_IDS[code]}")
                bits = got.view(torch.int32 if tout == F32 else torch.int16)
                assert bool((bits[m < 0] == 0).all()), "a dropped row is not +0 in every bit"


def test_a_map_selects_the_wave_kernel(dev):
    """fp32 LayerNorm of 256 x 4096: with an identity map the bits are those of the wave-per-row kernel (the first 256 rows of a
    257-row call), and the two kernels, which add in different orders, do differ in some last bit on these rows."""
    rows, C = 256, 4096
    x = N.norm_inputs(rows + 1, C, 11, F32)
    w, b = N.norm_weights(C, C)
    pads = ((0, 0),)
    wave, = _run_norm(dev, False, x, w, b, 1, pads=pads)
    wg, = _run_norm(dev, False, x[:rows], w, b, 1, pads=pads)
    mapped, = _run_norm(dev, False, x[:rows], w, b, 1, torch.arange(rows, dtype=torch.int32), pads=pads)
    assert torch.equal(mapped, wave[:rows])
    assert not torch.equal(wg, wave[:rows]), "the two kernels give the same bits here: this test cannot tell them apart"


# --------------------------------------------------------------------------------------------------------------- haff_row_stats
def _run_stats(dev, x, rms, code, pad):
    lib = _lib()
    rows, C = x.shape
    xg = E.widen(x, pad, R.NAN).to(dev)
    st = _out(rows, 2, F32, dev)
    assert lib.haff_row_stats(_p(xg), C + pad, _p(st), rows, C, N.EPS_RMS if rms else N.EPS_LN, int(rms), code, _s()) == 0
    full = st.cpu()
    assert bool((full[rows:] == R.SENT).all()), "stats past rows written"
    return full[:rows, 0], full[:rows, 1]


def _stats_case(dev, x, code, what, names=None):
    for rms in (False, True):
        (m, bm), (r, br) = N.expect_stats(x, rms, N.EPS_RMS if rms else N.EPS_LN)
        for pad in (0, 8):
            gm, gr = _run_stats(dev, x, rms, code, pad)
            if rms:
                assert bool((gm.view(torch.int32) == 0).all()), "the mean field of RMS statistics is not +0.0"
            for i in ([None] if names is None else range(len(names))):
                sel = slice(None) if i is None else slice(i, i + 1)
                tag = f"{what} rms {int(rms)} pad {pad}" + ("" if i is None else f" row '{names[i]}'")
                _check("row_stats mean", gm[sel], m[sel], bm[sel], tag)
                _check("row_stats rstd", gr[sel], r[sel], br[sel], tag)


@pytest.mark.parametrize("code", N.STATS_CODES, ids=_code_id)
@pytest.mark.parametrize("case", N.NORM_CASES, ids=_case_id)
def test_row_stats_shapes(dev, case, code):
    rows, C = case
    _stats_case(dev, N.norm_inputs(rows, C, C + rows, N.STATS_CODES[code]), code, f"{rows}x{C} {N.CODE_IDS[code]}")


@pytest.mark.parametrize("code", N.STATS_CODES, ids=_code_id)
def test_row_stats_value_rows(dev, code):
    for C in N.VALUE_C:
        for rms in (False, True):       # the f16 +-60000 row exists for RMS only: both row sets run both modes
            x, names = N.value_rows(C, C, N.STATS_CODES[code], rms)
            _stats_case(dev, x, code, f"C {C} {N.CODE_IDS[code]}", names)


# ------------------------------------------------------------------------------------------------------ haff_row_stats_finalize
@pytest.mark.parametrize("slots", N.FINALIZE_SLOTS)
@pytest.mark.parametrize("rows", N.FINALIZE_ROWS)
def test_row_stats_finalize_exact_partials(dev, rows, slots):
    """Partials whose double sums are exact, so the reference is exact rational arithmetic: mean and rstd within 2 fp32 ulps (+
    2^-52 (mean rstd)^2), at mean / std of 100 and 1000 too; a row whose E[x^2] - mean^2 is below zero is clamped."""
    lib = _lib()
    C = 64 * slots
    part, names = N.finalize_partials(rows, slots)
    mean, rstd, _ = N.finalize_exact(part, C, N.FINALIZE_EPS)
    bm, br = N.finalize_bounds(mean, rstd, C, N.FINALIZE_EPS)
    pg = torch.from_numpy(part).to(dev)
    st = _out(rows, 2, F32, dev)
    assert lib.haff_row_stats_finalize(_p(pg), _p(st), rows, slots, C, N.FINALIZE_EPS, _s()) == 0
    full = st.cpu()
    assert bool((full[rows:] == R.SENT).all()), "stats past rows written"
    for pattern in sorted(set(names)):
        idx = torch.tensor([i for i, n in enumerate(names) if n == pattern])
        for field, ref, bnd in (("mean", mean, bm), ("rstd", rstd, br)):
            _check(f"row_stats_finalize {field}", full[:rows, 0 if field == "mean" else 1][idx], torch.from_numpy(ref)[idx],
                   torch.from_numpy(bnd)[idx], f"rows {rows} slots {slots} C {C} '{pattern}'")


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_norm_refusals_leave_the_outputs_alone(dev):
    """A bad dtype code, C or ld not a multiple of 8, rows of 0, null w / b / stats -> HAFF_ERR_BAD_ARG; C = 8200 ->
    HAFF_ERR_UNSUPPORTED; after every refused call the outputs still hold the sentinel."""
    lib = _lib()
    C, rows = 64, 4
    x = torch.zeros((rows, 8208), dtype=F32, device=dev)
    w = torch.ones(8208, dtype=F32, device=dev)
    y, st = _out(rows, 8208, F32, dev), _out(rows, 2, F32, dev)
    s = _s()
    ln = lambda x_=x, ldx=C, y_=y, ldy=C, w_=w, b_=w, r=rows, c=C, code=1: lib.haff_layernorm(   # noqa: E731
        _p(x_), ldx, _p(y_), ldy, _p(w_), _p(b_), None, r, c, 1e-5, code, s)
    rm = lambda ldx=C, ldy=C, w_=w, r=rows, c=C, code=1: lib.haff_rmsnorm(_p(x), ldx, _p(y), ldy, _p(w_), r, c, 1e-6, code, s)   # noqa: E731
    rs = lambda ldx=C, st_=st, r=rows, c=C, code=1, rms=0: lib.haff_row_stats(_p(x), ldx, _p(st_), r, c, 1e-5, rms, code, s)   # noqa: E731
    assert ln() == 0 and rm() == 0 and rs() == 0            # the calls are well formed but for the one argument changed below
    y.fill_(R.SENT)
    st.fill_(R.SENT)
    for code in (4, -1, 7):
        assert ln(code=code) == BAD_ARG and rm(code=code) == BAD_ARG and rs(code=code) == BAD_ARG, code
    for code in (2, 4, -1):
        assert rs(code=code) == BAD_ARG and rs(code=code, rms=1) == BAD_ARG, f"haff_row_stats takes dtype code {code}"
    for c in (60, 0, -8):
        assert ln(c=c) == BAD_ARG and rm(c=c) == BAD_ARG and rs(c=c) == BAD_ARG, c
    assert ln(ldx=C + 4) == BAD_ARG and ln(ldy=C + 4) == BAD_ARG and rm(ldx=C + 4) == BAD_ARG and rm(ldy=C + 4) == BAD_ARG
    assert rs(ldx=C + 4) == BAD_ARG
    for r in (0, -1):
        assert ln(r=r) == BAD_ARG and rm(r=r) == BAD_ARG and rs(r=r) == BAD_ARG
    assert ln(w_=None) == BAD_ARG and ln(b_=None) == BAD_ARG and rm(w_=None) == BAD_ARG and rs(st_=None) == BAD_ARG
    assert ln(c=8200, ldx=8200, ldy=8200) == UNSUPPORTED and rm(c=8200, ldx=8200, ldy=8200) == UNSUPPORTED
    assert rs(c=8200, ldx=8200) == UNSUPPORTED
    pg = torch.zeros((rows, 2, 2), dtype=F32, device=dev)
    fin = lambda p_=pg, st_=st, r=rows, sl=2, c=128: lib.haff_row_stats_finalize(_p(p_), _p(st_), r, sl, c, 1e-6, s)   # noqa: E731
    assert fin(p_=None) == BAD_ARG and fin(st_=None) == BAD_ARG and fin(r=0) == BAD_ARG and fin(sl=0) == BAD_ARG and fin(c=0) == BAD_ARG
    torch.cuda.synchronize()
    assert bool((y.cpu() == R.SENT).all()) and bool((st.cpu() == R.SENT).all()), "a refused call wrote to its output"


# ------------------------------------------------------------------------------------------------------------ haff_resample_u8
def _tables(n_in, n_out, filt, dev):
    import haff  # noqa: F401
    from haff.preprocess import pil_resample_tables
    bounds, coeffs = pil_resample_tables(n_in, n_out, filt)
    assert int((bounds[:, 0] + bounds[:, 1]).max()) <= n_in and int(bounds.min()) >= 0
    return bounds, coeffs, torch.from_numpy(bounds).to(dev), torch.from_numpy(coeffs).to(dev)


def _resample(dev, img, out_hw, axis, filt, tail=64):
    """one pass through the C ABI -> (kernel output, restatement); the bytes after the output must keep the sentinel"""
    lib = _lib()
    B, H, W, _ = img.shape
    n_in, n_out = (W, out_hw[1]) if axis == 0 else (H, out_hw[0])
    bounds, coeffs, bg, cg = _tables(n_in, n_out, filt, dev)
    n = B * out_hw[0] * out_hw[1] * 3
    out = torch.full((n + tail,), 0xA5, dtype=torch.uint8, device=dev)
    assert lib.haff_resample_u8(_p(torch.from_numpy(img).to(dev)), _p(out), B, H, W, out_hw[0], out_hw[1], axis, _p(bg), _p(cg),
                                coeffs.shape[1], _s()) == 0
    full = out.cpu().numpy()
    assert (full[n:] == 0xA5).all(), "bytes after the output written"
    return full[:n].reshape(B, out_hw[0], out_hw[1], 3), N.resample_axis(img, axis, bounds, coeffs)


@pytest.mark.parametrize("filt", N.FILTERS)
@pytest.mark.parametrize("geom", N.GEOMETRIES, ids=lambda g: f"{g[0][0]}x{g[0][1]}-{g[1][0]}x{g[1][1]}")
def test_resample_equals_the_restatement(dev, geom, filt):
    """Every geometry (extents of 1, 4000 taps, single-axis calls), image kind and filter, B of 1 and 3: horizontal pass, then the
    vertical pass on the kernel's own intermediate, each array_equal to the restatement (which equals Pillow: the CPU test)."""
    (H, W), (Ho, Wo) = geom
    for kind in N.IMAGE_KINDS:
        for B in (1, 3):
            x = N.image(kind, B, H, W, seed=H + W + B)
            want = N.resize(x, (Ho, Wo), filt, lambda a, b, f: _tables(a, b, f, dev)[:2])
            if Wo != W:
                got, ref = _resample(dev, x, (H, Wo), 0, filt)
                assert np.array_equal(got, ref), (kind, B, "axis 0")
                x = got
            if Ho != H:
                got, ref = _resample(dev, x, (Ho, Wo), 1, filt)
                assert np.array_equal(got, ref), (kind, B, "axis 1")
                x = got
            assert np.array_equal(x, want), (kind, B)


@pytest.mark.parametrize("axis", [0, 1])
def test_resample_past_the_grid_cap(dev, axis):
    """65536 blocks of 256 threads and a ragged remainder: the grid-stride loop takes a second trip (axis 0 counts pixels, axis 1
    bytes)"""
    B, (H, W), out_hw = N.OVER_CAP[axis]
    got, ref = _resample(dev, N.image("random", B, H, W, seed=axis), out_hw, axis, "bicubic")
    assert np.array_equal(got, ref)


def test_resample_refusals(dev):
    lib = _lib()
    _, coeffs, bg, cg = _tables(4, 6, "bilinear", dev)
    img = torch.zeros((1, 4, 4, 3), dtype=torch.uint8, device=dev)
    out = torch.full((1 * 6 * 6 * 3,), 0xA5, dtype=torch.uint8, device=dev)
    k = coeffs.shape[1]
    call = lambda Ho, Wo, axis, b=bg, c=cg, ks=k, B=1: lib.haff_resample_u8(_p(img), _p(out), B, 4, 4, Ho, Wo, axis, _p(b), _p(c), ks, _s())   # noqa: E731
    assert call(6, 6, 0) == BAD_ARG, "axis 0 with Hout != Hin"
    assert call(6, 6, 1) == BAD_ARG, "axis 1 with Wout != Win"
    assert call(4, 6, 2) == BAD_ARG and call(4, 6, -1) == BAD_ARG, "axis 2"
    assert call(4, 6, 0, ks=0) == BAD_ARG and call(4, 6, 0, b=None) == BAD_ARG and call(4, 6, 0, c=None) == BAD_ARG
    assert call(4, 6, 0, B=0) == BAD_ARG and call(0, 6, 0) == BAD_ARG and call(4, 0, 0) == BAD_ARG
    torch.cuda.synchronize()
    assert bool((out.cpu() == 0xA5).all()), "a refused call wrote to its output"
    assert call(4, 6, 0) == 0 and call(6, 4, 1) == 0


@pytest.mark.parametrize("filt", N.FILTERS)
def test_frame_ingest_resize_with_one_side_matching(dev, filt):
    import haff  # noqa: F401
    from haff.preprocess import FrameIngest, pil_resample_tables
    ing = FrameIngest(dev)
    for (H, W), out in (((6, 5), (6, 11)), ((6, 5), (13, 5)), ((9, 8), (9, 3)), ((9, 8), (4, 8)), ((7, 5), (7, 5))):
        img = N.image("checkerboard", 2, H, W)
        got = ing.resize(torch.from_numpy(img).to(dev), out, filt).cpu().numpy()
        assert np.array_equal(got, N.resize(img, out, filt, pil_resample_tables)), ((H, W), out)


# ------------------------------------------------------------------------------------------------------ haff_clip_normalize_u8
def _lut():
    import haff  # noqa: F401
    from haff.preprocess import clip_normalize_lut
    return clip_normalize_lut()


def _clip(dev, frames, top, left, S, dtype, lut):
    lib = _lib()
    B, H, W, _ = frames.shape
    n = B * 3 * S * S
    out = torch.full((n + 64,), R.SENT, dtype=dtype, device=dev)
    assert lib.haff_clip_normalize_u8(_p(torch.from_numpy(frames).to(dev)), _p(out), B, H, W, top, left, S, _p(torch.from_numpy(lut).to(dev)),
                                      R.CODE[dtype], _s()) == 0
    full = out.cpu()
    assert bool((full[n:] == R.SENT).all()), "written past the output"
    return full[:n].reshape(B, 3, S, S)


@pytest.mark.parametrize("dtype", R.DTYPES, ids=lambda d: R.IDS[d])
def test_clip_normalize_every_lut_entry(dev, dtype):
    """Frames that hold every byte value in every channel; asymmetric top / left, S = 1, S equal to the frame, non-square frames:
    the f32 output is the LUT bit for bit, bf16 / f16 one rounding of it. A second LUT of distinct integers shows that all 3 x 256
    entries are the ones read."""
    luts = (_lut(), np.arange(768, dtype=np.float32).reshape(3, 256) - 300.0)
    for B, (H, W), top, left, S in N.CLIP_CASES:
        frames = N.every_byte_frame(B, H, W)
        for lut in luts:
            ref = torch.from_numpy(N.clip_normalize(frames, top, left, S, lut)).to(dtype)
            got = _clip(dev, frames, top, left, S, dtype, lut)
            assert torch.equal(got.view(torch.int32 if dtype == F32 else torch.int16), ref.view(torch.int32 if dtype == F32 else torch.int16)), \
                (B, H, W, top, left, S)
    B, (H, W), top, left, S = N.CLIP_CASES[0]
    assert len(np.unique(N.every_byte_frame(B, H, W)[0, top:top + S, left:left + S, 0])) == 256


def test_clip_normalize_past_the_grid_cap(dev):
    B, (H, W), top, left, S = N.CLIP_OVER_CAP
    frames = N.image("random", B, H, W, seed=3)
    lut = _lut()
    got = _clip(dev, frames, top, left, S, BF16, lut)
    assert torch.equal(got, torch.from_numpy(N.clip_normalize(frames, top, left, S, lut)).to(BF16))


def test_clip_normalize_refusals(dev):
    lib = _lib()
    frames = torch.zeros((1, 8, 9, 3), dtype=torch.uint8, device=dev)
    lut = torch.from_numpy(_lut()).to(dev)
    out = torch.full((3 * 8 * 8 + 8,), R.SENT, dtype=F32, device=dev)
    call = lambda top, left, S, code=1, l=lut, B=1: lib.haff_clip_normalize_u8(_p(frames), _p(out), B, 8, 9, top, left, S, _p(l), code, _s())   # noqa: E731
    for code in (2, 4, -1):
        assert call(0, 0, 8, code=code) == BAD_ARG, code
    assert call(1, 0, 8) == BAD_ARG and call(0, 2, 8) == BAD_ARG, "a crop overhanging on either axis"
    assert call(-1, 0, 4) == BAD_ARG and call(0, -1, 4) == BAD_ARG and call(0, 0, 0) == BAD_ARG
    assert call(0, 0, 8, l=None) == BAD_ARG and call(0, 0, 8, B=0) == BAD_ARG
    torch.cuda.synchronize()
    assert bool((out.cpu() == R.SENT).all()), "a refused call wrote to its output"
    assert call(0, 1, 8) == 0
