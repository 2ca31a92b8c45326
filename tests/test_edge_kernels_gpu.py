"""The data-movement kernels of csrc/elementwise.hip and the mask tail of csrc/sam_decoder.hip at their edges, each against the
float64 CPU restatement of tests/edge_ref.py (checked on its own by tests/test_edge_ref_cpu.py): non-square geometries (a swapped
w / h shows), extents of 1, shapes past the grid caps (the grid-stride loops iterate), NaN / inf / denormal / threshold-exact
values, row strides wider than the row, and every dtype code. No reference is built from another haff op, and everything is
compared on the CPU. Copies and single roundings are compared with torch.equal."""
import ctypes
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/edge_ref.py
import edge_ref as E   # noqa: E402

pytestmark = pytest.mark.gpu

BAD_ARG = -1
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
IDS = {torch.float32: "f32", torch.bfloat16: "bf16", torch.float16: "f16"}
_id = lambda v: IDS.get(v, None)   # noqa: E731


def _ops():
    import haff  # noqa: F401
    from haff import ops
    return ops


def _lib():
    import haff  # noqa: F401
    from haff.lib import load_library
    return load_library()


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _close(got, ref, rel, what):
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    scale = ref.abs().max().item() + 1e-12
    err = (got - ref).abs().max().item()
    print(f"{what}: max|err| {err:.4g}, scale {scale:.4g}, rel {err / scale:.3g} (bound {rel})")
    assert np.isfinite(err), f"{what}: non-finite output"
    assert err <= rel * scale, f"{what}: max|err|={err:.4g} vs scale {scale:.4g} (rel {err / scale:.3g} > {rel})"


# ---------------------------------------------------------------------------------------------------------------- argmax
@pytest.mark.parametrize("V", E.ARGMAX_V)
def test_argmax_rows_is_torch_argmax(dev, V):
    """First maximum, NaN above everything, first NaN first, never an index outside [0, V) — on a view whose row stride is wider
    than V with +inf to the right of it, and on the same rows packed. Only the output tensor is read."""
    ops = _ops()
    x, names = E.argmax_rows(V)
    ref = E.argmax(x)
    for what, xg in (("ld > V", E.widen(x, 13, E.INF).to(dev)[:, :V]), ("ld == V", x.contiguous().to(dev))):
        got = ops.argmax_rows(xg).cpu()
        bad = [(names[r], int(got[r]), int(ref[r])) for r in range(len(names)) if got[r] != ref[r]]
        assert torch.equal(got, ref), f"V={V} {what}: (row, got, expected) {bad}"


# -------------------------------------------------------------------------------------------------------- dtype dispatch
def _dtype_calls(dev):
    """(name, call(code) -> rc, output buffers) for every entry point of the data-movement group and haff_upscale_mask. Every
    buffer is valid and sized for fp32 rows, the widest type, so that a code which did reach a kernel stays inside them."""
    lib, s = _lib(), _stream()
    f = lambda *shape: torch.full(shape, 7.0, device=dev)   # noqa: E731
    calls = []
    x, out = f(1, 3, 16, 16), f(1, 768)
    calls.append(("haff_patchify_nchw in", lambda c: lib.haff_patchify_nchw(x.data_ptr(), out.data_ptr(), 1, 3, 16, 16, 16, 1, 1, 768, c, 1, s), [out]))
    calls.append(("haff_patchify_nchw out", lambda c: lib.haff_patchify_nchw(x.data_ptr(), out.data_ptr(), 1, 3, 16, 16, 16, 1, 1, 768, 1, c, s), [out]))
    calls.append(("haff_patchify_nchw both", lambda c: lib.haff_patchify_nchw(x.data_ptr(), out.data_ptr(), 1, 3, 16, 16, 16, 1, 1, 768, c, c, s), [out]))
    fr = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device=dev)
    m = (ctypes.c_float * 3)(*E.SAM_MEAN)
    sd = (ctypes.c_float * 3)(*E.SAM_STD)
    out_u8 = f(1, 768)
    calls.append(("haff_patchify_u8", lambda c: lib.haff_patchify_u8(fr.data_ptr(), out_u8.data_ptr(), 1, 16, 16, 16, 1, 1, 768, ctypes.cast(m, ctypes.c_void_p),
                                                                     ctypes.cast(sd, ctypes.c_void_p), c, s), [out_u8]))
    xi, oi = f(1, 2, 2, 8), f(4, 72)
    calls.append(("haff_im2col3x3", lambda c: lib.haff_im2col3x3(xi.data_ptr(), oi.data_ptr(), 1, 2, 2, 8, c, s), [oi]))
    ids = torch.tensor([[1, -200, 2]], device=dev)
    pos = torch.tensor([1], dtype=torch.int32, device=dev)
    emb, img, oe = f(4, 8), f(1, 1, 8), f(1, 3, 8)
    calls.append(("haff_embed_splice", lambda c: lib.haff_embed_splice(ids.data_ptr(), pos.data_ptr(), emb.data_ptr(), img.data_ptr(), oe.data_ptr(), 1, 3, 1, 8, c, s), [oe]))
    qkv, kc, vc = f(1, 48), f(1, 2, 16), f(1, 2, 16)
    cs = E.rope_table(2, 16).to(dev)
    p0 = torch.zeros(1, dtype=torch.int32, device=dev)
    calls.append(("haff_rope_cache", lambda c: lib.haff_rope_cache(qkv.data_ptr(), 48, kc.data_ptr(), vc.data_ptr(), cs.data_ptr(), 1, 1, 1, 1, 16, 1, 2, c, s), [qkv, kc, vc]))
    calls.append(("haff_rope_cache_rows", lambda c: lib.haff_rope_cache_rows(qkv.data_ptr(), 48, kc.data_ptr(), vc.data_ptr(), cs.data_ptr(), 1, 1, 1, 1, 16, p0.data_ptr(), 2, c, s),
                  [qkv, kc, vc]))
    a, b, oa = f(2, 8), f(2, 8), f(2, 8)
    calls.append(("haff_add_bcast", lambda c: lib.haff_add_bcast(a.data_ptr(), b.data_ptr(), oa.data_ptr(), 2, 8, 2, c, s), [oa]))
    xs, os_ = f(2, 4), f(2, 4)
    calls.append(("haff_softmax_rows", lambda c: lib.haff_softmax_rows(xs.data_ptr(), os_.data_ptr(), 2, 4, c, s), [os_]))
    up1, ln_w, ln_b, w2, b2, hy = (t.to(dev) for t in E.upscale_inputs(1, 1, 1, 3))
    ou = f(1, 4, 4)
    calls.append(("haff_upscale_mask", lambda c: lib.haff_upscale_mask(up1.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), w2.data_ptr(), b2.data_ptr(), hy.data_ptr(), ou.data_ptr(),
                                                                       1, 1, 1, 1e-6, c, s), [ou]))
    return calls


@pytest.mark.parametrize("code", [2, 4, -1])
def test_unknown_dtype_code_is_refused(dev, code):
    """No entry point treats a code it has no kernel for as fp32: it returns HAFF_ERR_BAD_ARG and writes nothing."""
    bad = []
    for name, call, outs in _dtype_calls(dev):
        rc = call(code)
        torch.cuda.synchronize()
        if rc != BAD_ARG or not all(bool((o == 7.0).all()) for o in outs):
            bad.append((name, rc))
    assert not bad, f"dtype code {code} accepted by (entry point, return code): {bad}"


def test_patchify_nchw_refuses_the_pairs_it_has_no_kernel_for(dev):
    lib, s = _lib(), _stream()
    x, out = torch.zeros((1, 3, 16, 16), device=dev), torch.full((1, 768), 7.0, device=dev)
    for i, o in ((3, 0), (0, 3), (3, 1)):
        assert lib.haff_patchify_nchw(x.data_ptr(), out.data_ptr(), 1, 3, 16, 16, 16, 1, 1, 768, i, o, s) == BAD_ARG, (i, o)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---------------------------------------------------------------------------------------------------------- upscale_mask
def _up1_on_device(up1, dtype, dev):
    """up1 in `dtype` on the device, as the first half of an allocation twice its size: a kernel that took 16-bit rows for
    fp32 ones would still read inside it."""
    buf = torch.zeros((2 * up1.shape[0], up1.shape[1]), dtype=dtype, device=dev)
    buf[:up1.shape[0]] = up1.to(dtype)
    return buf[:up1.shape[0]]


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("n,h,w", [(1, 1, 1), (3, 3, 5), (2, 5, 3), (1, 16, 16)])
def test_upscale_mask_non_square(dev, n, h, w, dtype):
    """LayerNorm2d -> GELU -> ConvT(64 -> 32) -> GELU -> dot with hyper against float64, from the same rounded up1 the kernel reads;
    h != w shows a swapped pix % w or yy * W4 + xx, (1, 1, 1) is four units in a 256-thread block."""
    ops = _ops()
    up1, ln_w, ln_b, w2, b2, hyper = E.upscale_inputs(n, h, w, 20 + h)
    ug = _up1_on_device(up1, dtype, dev)
    got = ops.upscale_mask(ug, *(t.to(dev) for t in (ln_w, ln_b, w2, b2, hyper)), n, h, w)
    ref = E.upscale_mask(ug.cpu().float(), ln_w, ln_b, w2, b2, hyper, n, h, w)
    assert got.shape == (n, 4 * h, 4 * w)
    _close(got, ref, 1e-4 if dtype == torch.float32 else 3e-2, f"upscale_mask {n}x{h}x{w} {IDS[dtype]}")


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_upscale_mask_constant_pixels(dev, dtype):
    """Pixels whose 64 channels are all equal: v - mean is exactly 0, so the result depends on ln_b alone — the constant 1000 gives
    the same bits as the constant 0, and both match float64 at the fp32 tolerance (1000 and the random rest are exact in all three
    types' own rounding, and the reference reads the rounded rows)."""
    ops = _ops()
    n, h, w = 2, 3, 5
    up1, ln_w, ln_b, w2, b2, hyper = E.upscale_inputs(n, h, w, 31)
    units = up1.view(n * h * w * 4, 64)                    # one (pixel, tap) unit per row
    const = torch.arange(units.shape[0]) % 3 == 0
    outs = []
    for value in (1000.0, 0.0):
        units[const] = value
        ug = _up1_on_device(up1, dtype, dev)
        outs.append(ops.upscale_mask(ug, *(t.to(dev) for t in (ln_w, ln_b, w2, b2, hyper)), n, h, w).cpu())
        ref = E.upscale_mask(ug.cpu().float(), ln_w, ln_b, w2, b2, hyper, n, h, w)
        _close(outs[-1], ref, 1e-4 if dtype == torch.float32 else 3e-2, f"upscale_mask constant {value} {IDS[dtype]}")
    assert torch.equal(outs[0], outs[1])
    # the constant units alone, at the fp32 tolerance in every input type: their value does not pass through the 16-bit rounding
    up_const = torch.zeros((n * h * w, 256))
    ref = E.upscale_mask(up_const, ln_w, ln_b, w2, b2, hyper, n, h, w)
    for value in (1000.0, 0.0):
        got = ops.upscale_mask(_up1_on_device(up_const + value, dtype, dev), *(t.to(dev) for t in (ln_w, ln_b, w2, b2, hyper)), n, h, w)
        _close(got, ref, 1e-4, f"upscale_mask all-constant {value} {IDS[dtype]}")


# ------------------------------------------------------------------------------------------------------- resize_bilinear
@pytest.mark.parametrize("case", E.RESIZE_CASES + (E.RESIZE_BIG,), ids=lambda c: f"{c[1]}-{c[2]}-{c[3]}")
def test_resize_bilinear_edges(dev, case):
    """F.interpolate(bilinear, align_corners=False) of the float64 crop, within edge_ref.resize_tol (derived there). Everything
    outside the crop is NaN: a finite output shows that nothing there is read. The last case is past the 16384-block cap."""
    ops = _ops()
    _, _, crop, out = case
    x = E.resize_source(case, 11)
    ref = E.resize_bilinear(x, crop, out)
    tol = E.resize_case_tol(x, crop)
    got = ops.resize_bilinear(x.to(dev), crop, out).cpu()
    assert got.shape == ref.shape
    assert bool(torch.isfinite(got).all()), "read outside the crop"
    err = E.max_err(got, ref)
    print(f"resize {case}: max|err| {err:.4g}, bound {tol:.4g}")
    assert err <= tol, (err, tol)


# ------------------------------------------------------------------------------------------------------------ thresholds
TH = 0.4054651          # logit(0.6)
TH8 = (0.0, TH, -TH, 2.0, -2.0, 1e-45, E.INF, -E.INF)


@pytest.mark.parametrize("total", E.THRESHOLD_TOTALS)
def test_threshold_masks_exact(dev, total):
    ops = _ops()
    for k, th in enumerate((0.0, TH, -E.INF)):
        x = E.threshold_values(total, (th, 0.0), 3 * total + k)
        got = ops.threshold_masks(x.to(dev), th).cpu()
        assert torch.equal(got, E.threshold(x, (th,), 255)[0]), (total, th)


def test_threshold_masks_past_the_cap(dev):
    ops = _ops()
    total = 16384 * 256 + 5
    x = E.threshold_values(total, (TH, 0.0), 1)
    assert torch.equal(ops.threshold_masks(x.to(dev), TH).cpu(), E.threshold(x, (TH,), 255)[0])


def _taxonomies(dev):
    """(name, taxonomy or None, blank_class, open?) — argmax ties go to the first class"""
    t = lambda *v: torch.tensor(v, dtype=torch.float32, device=dev)   # noqa: E731
    return (("none", None, 2, True), ("open", t(0.1, 0.2, 0.6, 0.1), 1, True), ("blanked", t(0.1, 0.2, 0.6, 0.1), 2, False),
            ("tie, first class is blank", t(0.3, 0.3, 0.2, 0.2), 0, False), ("tie, second class is blank", t(0.3, 0.3, 0.2, 0.2), 1, True),
            ("last class", t(0.1, 0.2, 0.3, 0.4), 3, False))


@pytest.mark.parametrize("total", E.THRESHOLD_TOTALS)
def test_gate_threshold_masks_exact(dev, total):
    """(x > th) * on for every threshold, all-zero planes when the taxonomy's first maximum is the blank class; total % 4 in
    {0, 1, 2, 3} and total < 4 (the float4 body and the byte tail), values at and beside each threshold, +-0, denormals, +-inf, NaN."""
    ops = _ops()
    for ths in ((TH,), TH8):
        x = E.threshold_values(total, ths, 5 * total + len(ths))
        xg = x.to(dev)
        for on in (0, 1, 255):
            ref = E.threshold(x, ths, on)
            for name, tax, blank, is_open in _taxonomies(dev):
                got = ops.gate_threshold_masks(xg, ths, on_value=on, taxonomy=tax, blank_class=blank).cpu()
                assert got.shape == ref.shape
                assert torch.equal(got, ref if is_open else torch.zeros_like(ref)), (total, len(ths), on, name)


@pytest.mark.parametrize("total", E.THRESHOLD_TOTALS)
def test_gate_threshold_masks_leaves_the_padding(dev, total):
    """The bytes of each plane between total and plane_stride are not the kernel's to write."""
    lib = _lib()
    ths = (0.0, TH, -E.INF)
    stride = (total + 3) // 4 * 4 + 8
    x = E.threshold_values(total, ths, total)
    xg = x.to(dev)
    planes = torch.full((len(ths), stride), 0xAB, dtype=torch.uint8, device=dev)
    arr = (ctypes.c_float * len(ths))(*ths)
    rc = lib.haff_gate_threshold_masks(xg.data_ptr(), planes.data_ptr(), total, stride, ctypes.cast(arr, ctypes.c_void_p), len(ths), 255, 0, -1,
                                       _stream())
    assert rc == 0
    got = planes.cpu()
    assert torch.equal(got[:, :total], E.threshold(x, ths, 255))
    assert bool((got[:, total:] == 0xAB).all())


def test_gate_threshold_masks_past_the_cap(dev):
    ops = _ops()
    total = 8192 * 256 * 4 + 7
    ths = (TH, 0.0)
    x = E.threshold_values(total, ths, 2)
    got = ops.gate_threshold_masks(x.to(dev), ths, on_value=255).cpu()
    assert torch.equal(got, E.threshold(x, ths, 255))


def test_gate_threshold_masks_refusals(dev):
    lib, s = _lib(), _stream()
    x = torch.zeros(64, device=dev)
    planes = torch.full((9, 64), 0xAB, dtype=torch.uint8, device=dev)
    arr = (ctypes.c_float * 9)(*([0.0] * 9))
    th = ctypes.cast(arr, ctypes.c_void_p)
    call = lambda xp, total, stride, n_th: lib.haff_gate_threshold_masks(xp, planes.data_ptr(), total, stride, th, n_th, 255, 0, -1, s)   # noqa: E731
    assert x.data_ptr() % 16 == 0
    assert call(x.data_ptr(), 16, 64, 8) == 0                        # the same call is accepted with 8 thresholds
    assert call(x.data_ptr(), 16, 64, 9) == BAD_ARG                  # n_th = 9
    assert call(x.data_ptr(), 16, 12, 1) == BAD_ARG                  # plane_stride < total
    assert call(x.data_ptr(), 16, 18, 1) == BAD_ARG                  # plane_stride % 4 != 0
    assert call(x.data_ptr() + 4, 16, 16, 1) == BAD_ARG              # logits not 16-byte aligned
    torch.cuda.synchronize()
    assert bool((planes.cpu()[8] == 0xAB).all()) and bool((planes.cpu()[:8, 16:] == 0xAB).all())


# ---------------------------------------------------------------------------------------------------------- softmax_rows
@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("rows", [1, 64, 65, 130])
def test_softmax_rows_edges(dev, rows, dtype):
    """float64 softmax of the same rounded logits, absolute 1e-6; -inf entries give exactly 0; the row with one +inf is NaN
    throughout, which is what exp(x - max) / sum gives (edge_ref.softmax_rows) — no special rule. 65 and 130 rows: a second and a
    third 64-row block."""
    ops = _ops()
    for C in (1, 4, 7):
        x = E.softmax_rows_input(rows, C, rows + C).to(dtype)
        ref = E.softmax_rows(x.float())
        got = ops.softmax_rows(x.to(dev)).cpu().double()
        assert torch.equal(torch.isnan(got), torch.isnan(ref)), (rows, C)
        err = (torch.nan_to_num(got) - torch.nan_to_num(ref)).abs().max().item()
        print(f"softmax {rows}x{C} {IDS[dtype]}: max|err| {err:.3g}")
        assert err <= 1e-6, (rows, C, err)
        gone = torch.isinf(x.float()) & (x.float() < 0) & ~torch.isnan(ref)
        assert bool((got[gone] == 0).all())


# --------------------------------------------------------------------------------------------------------------- gathers
PAIRS = ((torch.bfloat16, torch.bfloat16), (torch.float32, torch.bfloat16), (torch.float32, torch.float32), (torch.bfloat16, torch.float32),
         (torch.float16, torch.float16), (torch.float32, torch.float16))


@pytest.mark.parametrize("tin,tout", PAIRS, ids=lambda t: IDS[t])
def test_patchify_nchw_non_square(dev, tin, tout):
    """F.unfold rows, the values converted once to the output type: gh != gw, an input larger than the patch grid (the rest is
    ignored), CLIP's 14-pixel patches with K padded to 592."""
    ops = _ops()
    for P, gh, gw, Kp, H, W in ((16, 3, 5, 768, 50, 83), (14, 2, 3, 592, 31, 42), (14, 3, 2, 592, 42, 28)):
        x = E.rand((2, 3, H, W), P + gh).to(tin)
        got = ops.patchify_nchw(x.to(dev), P, gh, gw, Kp, tout).cpu()
        assert torch.equal(got, E.patchify_nchw(x, P, gh, gw, Kp, tout)), (P, gh, gw)


def test_patchify_nchw_past_the_cap(dev):
    ops = _ops()
    x = E.rand((1, 3, 1024, 1024), 4).to(torch.bfloat16)          # 3.1 M outputs > 8192 x 256
    got = ops.patchify_nchw(x.to(dev), 16, 64, 64, 768, torch.bfloat16).cpu()
    assert torch.equal(got, E.patchify_nchw(x, 16, 64, 64, 768, torch.bfloat16))


@pytest.mark.parametrize("tout", DTYPES, ids=_id)
def test_patchify_u8_pads_and_normalises(dev, tout):
    """(u8 - mean) / std in float64, zero where the frame does not reach: frames smaller than the 2 x 3 patch canvas in both
    directions, larger in both, and mixed. fp32 output within 2 ulp: the subtraction and the division are each correctly rounded
    (relative error < 2.0001 * 2^-24 together) and one ulp is at least 2^-24 * |v|. bf16 / f16 output: that value rounded once
    (test_edge_ref_cpu shows that rounding the float64 or the fp32 value gives the same for all 768 values there are)."""
    ops = _ops()
    P, gh, gw, Kp = 16, 2, 3, 776
    g = torch.Generator().manual_seed(5)
    for Hf, Wf in ((20, 30), (40, 60), (20, 60), (40, 30), (32, 48)):
        fr = torch.randint(0, 256, (2, Hf, Wf, 3), dtype=torch.uint8, generator=g)
        ref = E.patchify_u8(fr, P, gh, gw, Kp, E.SAM_MEAN, E.SAM_STD)
        got = ops.patchify_u8(fr.to(dev), P, gh, gw, Kp, E.SAM_MEAN, E.SAM_STD, tout).cpu()
        assert got.shape == ref.shape
        assert bool((got[ref == 0] == 0).all()), "padding is not zero"
        if tout == torch.float32:
            over = ((got.double() - ref).abs() - 2 * E.ulp32(ref)).max().item()
            assert over <= 0, (Hf, Wf, over)
        else:
            assert torch.equal(got, ref.to(tout)), (Hf, Wf)


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_im2col3x3_edges(dev, dtype):
    """F.unfold(3, padding 1) with columns re-ordered to (ky, kx, c), bit for bit: H or W of 1 (every tap but the centre row /
    column is padding), H != W."""
    ops = _ops()
    for shape in ((1, 1, 1, 8), (2, 1, 5, 16), (1, 5, 1, 8), (2, 6, 7, 16)):
        x = E.rand(shape, sum(shape)).to(dtype)
        assert torch.equal(ops.im2col3x3(x.to(dev)).cpu(), E.im2col3x3(x)), shape


def test_im2col3x3_past_the_cap(dev):
    ops = _ops()
    x = E.rand((2, 64, 64, 256), 6).to(torch.bfloat16)            # 2.36 M units of 8 > 8192 x 256
    got = ops.im2col3x3(x.to(dev)).cpu()
    assert torch.equal(got, E.im2col3x3(x, via=torch.float32))     # a copy: fp32 holds bf16 exactly, at half the memory of float64


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("Hd", [8, 1024, 1032, 5120])
def test_embed_splice_edges(dev, Hd, dtype):
    """Sentinel at 0 and at L - 1, n_img = 1; Hd = one thread, exactly one 128 x 8 trip, a one-thread tail trip, five trips."""
    ops = _ops()
    V, L = 11, 6
    emb = E.rand((V, Hd), Hd).to(dtype)
    for n_img in (1, 3):
        g = torch.Generator().manual_seed(n_img)
        ids = torch.randint(0, V, (3, L), generator=g)
        pos = torch.tensor([0, L - 1, 2], dtype=torch.int32)
        ids[torch.arange(3), pos.long()] = -200
        img = E.rand((3, n_img, Hd), Hd + n_img).to(dtype)
        got = ops.embed_splice(ids.to(dev), pos.to(dev), emb.to(dev), img.to(dev)).cpu()
        assert torch.equal(got, E.embed_splice(ids, pos, emb, img)), n_img


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
def test_add_bcast_edges(dev, dtype):
    """a[r] + b[r % mod]: the fp32 sum, rounded once to the storage type; mod of 1, 3, rows and one that does not divide rows;
    C = 8 (one unit per row); in place as sam.py calls it."""
    ops = _ops()
    for rows, mod, C in ((6, 1, 8), (6, 3, 8), (6, 6, 24), (7, 3, 8), (10, 4, 264)):
        a, b = E.rand((rows, C), rows + mod).to(dtype), E.rand((mod, C), C + mod).to(dtype)
        ref = E.add_bcast(a, b, mod)
        assert torch.equal(ops.add_bcast(a.to(dev), b.to(dev), mod=mod).cpu(), ref), (rows, mod, C)
        ag = a.to(dev)
        out = ops.add_bcast(ag, b.to(dev), mod=mod, out=ag)
        assert out.data_ptr() == ag.data_ptr() and torch.equal(ag.cpu(), ref), ("in place", rows, mod, C)


def test_add_bcast_past_the_cap(dev):
    ops = _ops()
    a, b = E.rand((66000, 256), 7).to(torch.bfloat16), E.rand((4096, 256), 8).to(torch.bfloat16)   # 2.112 M units > 8192 x 256
    ag = a.to(dev)
    ops.add_bcast(ag, b.to(dev), out=ag)
    assert torch.equal(ag.cpu(), E.add_bcast(a, b, 4096))


@pytest.mark.parametrize("dtype", DTYPES, ids=_id)
@pytest.mark.parametrize("d", [16, 128])
def test_rope_cache_grouped_heads_and_edges(dev, d, dtype):
    """Hkv < Hq, a row stride wider than q | k | v, pos0 + Tq == Tmax, ragged starts including 0 and Tmax - Tq: q and k against the
    float64 rotation (the tolerances of test_embed_splice_rope_argmax; f16 rounds once to 11 bits: 2^-10 of the scale), the k cache
    the same bits as the rotated k, the v cache the same bits as v, and nothing else written."""
    ops = _ops()
    B, Tq, Hq, Hkv, Tmax = 3, 3, 4, 2, 8
    width = (Hq + 2 * Hkv) * d
    tol = {torch.float32: 1e-6, torch.bfloat16: 1e-2, torch.float16: 2.0 ** -10}[dtype]
    cs = E.rope_table(Tmax, d)
    for starts in (None, [0, Tmax - Tq, 2]):
        qkv = E.widen(E.rand((B * Tq, width), d + 1), 8, 5.0).to(dtype)
        qg = qkv.to(dev)
        kc = torch.full((B, Tmax, Hkv * d), 7.0, dtype=dtype, device=dev)
        vc = torch.full((B, Tmax, Hkv * d), 7.0, dtype=dtype, device=dev)
        view = qg[:, :width]
        assert view.stride(0) == width + 8
        if starts is None:
            starts_ = [Tmax - Tq] * B
            ops.rope_cache(view, kc, vc, cs.to(dev), B, Tq, Hq, Hkv, d, Tmax - Tq)
        else:
            starts_ = starts
            ops.rope_cache_rows(view, kc, vc, cs.to(dev), B, Tq, Hq, Hkv, d, torch.tensor(starts, dtype=torch.int32, device=dev))
        q, k, v = E.rope_cache(qkv.float(), cs, B, Tq, Hq, Hkv, d, starts_)
        out = qg.cpu()
        got = out[:, :width].reshape(B, Tq, Hq + 2 * Hkv, d)
        _close(got[:, :, :Hq], q, tol, f"rope q d={d} {IDS[dtype]}")
        _close(got[:, :, Hq:Hq + Hkv], k, tol, f"rope k d={d} {IDS[dtype]}")
        assert torch.equal(got[:, :, Hq + Hkv:], qkv[:, :width].reshape(B, Tq, -1, d)[:, :, Hq + Hkv:]), "v columns of qkv changed"
        assert bool((out[:, width:] == 5.0).all()), "columns right of q | k | v written"
        kcc, vcc = kc.cpu().view(B, Tmax, Hkv, d), vc.cpu().view(B, Tmax, Hkv, d)
        written = torch.zeros((B, Tmax), dtype=torch.bool)
        for b in range(B):
            written[b, starts_[b]:starts_[b] + Tq] = True
            assert torch.equal(kcc[b, starts_[b]:starts_[b] + Tq], got[b, :, Hq:Hq + Hkv]), "k cache is not the rotated k"
            assert torch.equal(vcc[b, starts_[b]:starts_[b] + Tq].double(), v[b]), "v cache is not v"
        assert bool((kcc[~written] == 7.0).all()) and bool((vcc[~written] == 7.0).all()), "cache written outside pos0 .. pos0 + Tq"
