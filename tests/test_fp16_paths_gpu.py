"""f16 routes of the fp16 mode at the geometries where the model reaches them, each an f16 counterpart of a bf16 test in
test_ops_gpu.py.

GEMM routes use exact operands: small integers (|v| <= 4) and fp32 biases / LayerNorm statistics that are integers or powers of
two, so every partial sum and every epilogue step is exact in fp32. The f16 output must then EQUAL torch's conversion of the exact
result (one rounding), whatever the tile, the K order or the dispatch; activations that are not exact (GELU, SwiGLU) are held to
one f16 ulp of an fp64 reference. Attention: fp64 torch on the same f16 operands and f16-rounded rel-pos tables.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

F16 = torch.float16


def _ops():
    import haff  # noqa: F401
    from haff import ops
    return ops


def _ints(shape, seed, lo=-4, hi=4):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _h(t, dev):
    return t.to(F16).to(dev)


def _ulp16(x):
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -14)))
    return torch.pow(2.0, e - 10)


def _within_ulp(got, ref, what, floor=0.0):
    """|got - ref| <= one f16 ulp of ref (+ floor: fp32 cancellation in rotations)"""
    err = (got.double().cpu() - ref.cpu()).abs()
    assert torch.isfinite(got).all(), what
    assert (err <= _ulp16(ref.cpu()) + floor).all(), (what, err.max().item())


def _within_gelu(got, ref, what):
    """GELU outputs: one f16 ulp, plus the kernel's GELU approximation. gemm_act clamps erf's argument at 3, so below
    x = -3 sqrt 2 it returns x (1 - erf(3)) / 2 = -1.1e-5 |x| instead of ~0 (measured max|err| 1.2e-2 at |x| ~ 1000 here): the
    bound adds 2^-16 of the output scale, a quarter of an f16 half-ulp at that scale."""
    err = (got.double().cpu() - ref.cpu()).abs()
    assert torch.isfinite(got).all(), what
    assert (err <= _ulp16(ref.cpu()) + 2.0 ** -16 * ref.abs().max().item()).all(), (what, err.max().item())


def _swiglu_ref(acc):
    M, N = acc.shape
    a = acc.view(M, N // 32, 2, 16)
    return (F.silu(a[:, :, 0]) * a[:, :, 1]).reshape(M, N // 2)


# --- 192-row tile ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("M,N,K", [(2808, 4096, 4096), (1500, 1280, 1280)])
def test_f16_gemm_192_row_tile(dev, M, N, K):
    """gemm_bf16_kernel<192, 256, ..., F16> (HAFF_SPEC192 instances): the auto choice == tile_cfg=3 bit for bit, == the exact
    product through the residual / bias epilogues, SwiGLU within one f16 ulp, and the gather (haff_gemm_f16_gather) exact."""
    ops = _ops()
    a, w = _ints((M, K), 1), _ints((N, K), 2)
    bias, resid = _ints((N,), 3) * 64, _ints((M, N), 4) * 16
    exact = a @ w.T
    x, wt, b, r = _h(a, dev), _h(w, dev), bias.float().to(dev), _h(resid, dev)
    got = ops.linear(x, wt, bias=b, resid=r)
    assert torch.equal(got, ops.linear(x, wt, bias=b, resid=r, tile_cfg=3))
    assert torch.equal(got.cpu(), (exact + bias + resid).float().to(F16))
    for kw, ref in ((dict(), exact), (dict(bias=b), exact + bias), (dict(resid=r), exact + resid)):
        assert torch.equal(ops.linear(x, wt, tile_cfg=3, **kw).cpu(), ref.float().to(F16)), sorted(kw)
    ws = _h(w * 2.0 ** -6, dev)
    _within_ulp(ops.linear(x, ws, swiglu=True, tile_cfg=3), _swiglu_ref(exact * 2.0 ** -6), "192-row tile swiglu")
    g = torch.Generator().manual_seed(5)
    a_map = torch.randint(0, M, (M,), generator=g).to(torch.int32)
    got = ops.linear(x, wt, bias=b, a_map=a_map.to(dev))
    assert torch.equal(got.cpu(), (exact[a_map.long()] + bias).float().to(F16))


@pytest.mark.parametrize("M,N,K", [(1500, 1280, 1280), (401, 512, 128)])
def test_f16_gemm_192_row_tile_row_maps(dev, M, N, K):
    """192-row tile with an output row map (dropped rows, ragged last M-tile), GELU / residual epilogues: == the 128 x 128 tile
    bit for bit and == exact (GELU within one ulp); gather + row map."""
    ops = _ops()
    a, w = _ints((M, K), 11), _ints((N, K), 12)
    bias = _ints((N,), 13) * 8
    exact = a @ w.T + bias
    g = torch.Generator().manual_seed(14)
    rows_out = M + 37
    perm = torch.randperm(rows_out, generator=g)[:M]
    drop = torch.rand((M,), generator=g) < 0.07
    rmap = torch.where(drop, torch.full((M,), -1), perm).to(torch.int32)
    resid = _ints((rows_out, N), 15) * 4
    x, wt, b, rm = _h(a, dev), _h(w, dev), bias.float().to(dev), rmap.to(dev)
    keep = ~drop
    for act in (0, 1):
        for use_res in (False, True):
            outs = []
            for cfg in (3, 1):
                out = torch.full((rows_out, N), 5.0, dtype=F16, device=dev)
                ops.linear(x, wt, bias=b, act=act, resid=_h(resid, dev) if use_res else None, row_map=rm, out=out, tile_cfg=cfg)
                outs.append(out)
            assert torch.equal(outs[0], outs[1]), (act, use_res)
            exp = torch.full((rows_out, N), 5.0, dtype=torch.float64)
            y = F.gelu(exact) if act else exact
            exp[rmap[keep].long()] = y[keep] + (resid[rmap[keep].long()] if use_res else 0.0)
            if act:
                _within_gelu(outs[0], exp, "192-row tile, row map, gelu")
            else:
                assert torch.equal(outs[0].cpu(), exp.float().to(F16)), use_res
    a_map = torch.randint(0, M, (M,), generator=g).to(torch.int32)
    got = ops.linear(x, wt, bias=b, a_map=a_map.to(dev), row_map=rm, out=torch.full((rows_out, N), 5.0, dtype=F16, device=dev))
    exp = torch.full((rows_out, N), 5.0, dtype=torch.float64)
    exp[rmap[keep].long()] = (a[a_map.long()] @ w.T + bias)[keep]
    assert torch.equal(got.cpu(), exp.float().to(F16))


# --- specialised 256 x 256 instances ----------------------------------------------------------------------------------------

def _ln_operands(M, N, K, seed):
    """integer activations / folded weights, LayerNorm statistics {mean: integer, rstd: power of two}, colsum = row sums of w:
    rstd * (acc - mean * colsum) + bias is exact in fp32"""
    a, w = _ints((M, K), seed), _ints((N, K), seed + 1)
    mean = _ints((M,), seed + 2, -2, 2)
    rstd = torch.pow(2.0, _ints((M,), seed + 3, -3, 1))
    colsum = w.sum(1)
    bias = _ints((N,), seed + 4) * 4
    ref = rstd[:, None] * (a @ w.T - mean[:, None] * colsum[None, :]) + bias
    st = torch.stack([mean, rstd], 1).float().contiguous()
    return a, w, st, colsum.float(), bias.float(), ref


def test_f16_gemm_specialised_instances(dev):
    """The HAFF_SPEC instances the fp16 mode reaches (all but GF_RES32), in f16: GF_BIAS|GF_LN|GF_CSUM (q|k|v, folded norm),
    ... |GELU (folded lin1), and the ragged-M plain / bias / residual / SwiGLU / quick-GELU instances (Llama prefill, CLIP) at
    M = 582 (a ragged last M-tile). Exact (activations within one f16 ulp). The others have tests of their own:
    GF_MAP|GF_HM in test_f16_linear_heads_scatter, GF_BIAS|GF_RES|GF_STAT in test_f16_linear_rowstats, GF_ROPE|GF_RAGM in
    test_fp16_edges_gpu.py::test_f16_rowstats_and_qkv_rope_exact_edges."""
    ops = _ops()
    M, N, K = 512, 768, 256
    a, w, st, cs, bias, ref = _ln_operands(M, N, K, 20)
    x, wt = _h(a, dev), _h(w, dev)
    got = ops.linear(x, wt, bias=bias.to(dev), ln_stats=st.to(dev), ln_colsum=cs.to(dev))
    assert torch.equal(got.cpu(), ref.float().to(F16))
    got = ops.linear(x, wt, bias=bias.to(dev), act=1, ln_stats=st.to(dev), ln_colsum=cs.to(dev))
    _within_gelu(got, F.gelu(ref), "LN + CSUM + GELU")
    # ragged-M instances
    M = 582
    a, w = _ints((M, K), 30), _ints((N, K), 31)
    exact = a @ w.T
    bias, resid = _ints((N,), 32) * 8, _ints((M, N), 33) * 16
    x, wt, b, r = _h(a, dev), _h(w, dev), bias.float().to(dev), _h(resid, dev)
    for kw, want in ((dict(), exact), (dict(bias=b), exact + bias), (dict(resid=r), exact + resid),
                     (dict(bias=b, resid=r), exact + bias + resid)):
        for cfg in (0, 2):
            assert torch.equal(ops.linear(x, wt, tile_cfg=cfg, **kw).cpu(), want.float().to(F16)), (sorted(kw), cfg)
    y = exact / 64 + bias
    _within_ulp(ops.linear(_h(a / 8, dev), _h(w / 8, dev), bias=b, act=ops.ACT_QUICK_GELU, tile_cfg=2), y * torch.sigmoid(1.702 * y),
                "ragged quick-gelu")
    ws = w * 2.0 ** -6
    _within_ulp(ops.linear(x, _h(ws, dev), swiglu=True, tile_cfg=2), _swiglu_ref(a @ ws.T), "ragged swiglu")


@pytest.mark.parametrize("fold", [False, True])
@pytest.mark.parametrize("M,K,H,d", [(512, 128, 16, 80), (1024, 1280, 16, 80)])
def test_f16_linear_heads_scatter(dev, M, K, H, d, fold):
    """haff_gemm_f16_heads (the windowed q|k|v written head-major, sam.py's ViT-H default): columns part * H * d + h * d + c of
    row m land at planes[part][w][h][t][c] for row_map[m] = w * H * n_tok + t, dropped rows (-1) and unaddressed slots
    untouched; == the token-major product bit for bit and == exact, with the folded LayerNorm (GF_MAP|GF_HM) and without."""
    ops = _ops()
    ntok = 196
    nwin = (M + ntok - 1) // ntok + 1
    N = 3 * H * d
    if fold:
        a, w, st, cs, bias, exact = _ln_operands(M, N, K, 70)
        kw = dict(ln_stats=st.to(dev), ln_colsum=cs.to(dev))
    else:
        a, w = _ints((M, K), 70), _ints((N, K), 71)
        bias = _ints((N,), 72).float()
        exact = a @ w.T + bias
        kw = {}
    x, wt, b = _h(a, dev), _h(w, dev), bias.to(dev)
    g = torch.Generator().manual_seed(73)
    slots = torch.randperm(nwin * ntok, generator=g)[:M]
    keep = torch.rand((M,), generator=g) > 0.1
    rmap = torch.where(keep, (slots // ntok) * (H * ntok) + slots % ntok, torch.full((M,), -1)).to(torch.int32).to(dev)
    assert ops.linear_heads_supported(M, N, K, d, H, F16)
    planes = torch.full((3, nwin + 1, H, ntok, d), 7.0, dtype=F16, device=dev)
    ops.linear_heads(x, wt, b, rmap, planes, d, H, (nwin + 1) * H * ntok * d, ntok * d, **kw)
    tok = ops.linear(x, wt, bias=b, tile_cfg=0 if fold else 2, **kw)
    assert torch.equal(tok.cpu(), exact.float().to(F16))
    exp = torch.full_like(planes, 7.0)
    mk = keep.to(dev)
    wi, ti = (slots // ntok).to(dev)[mk], (slots % ntok).to(dev)[mk]
    ref = tok.view(M, 3, H, d)
    for part in range(3):
        exp[part, wi, :, ti] = ref[mk, part]
    assert torch.equal(planes, exp)


@pytest.mark.parametrize("M,N,K", [(300, 256, 128), (1000, 1280, 1280), (70, 96, 64)])
def test_f16_linear_gather_rows(dev, M, N, K):
    """haff_gemm_f16_gather: logical row m reads x[a_map[m]], with bias and residual, in place as SAM's proj uses it: exact."""
    ops = _ops()
    R = M + 57
    a, w = _ints((R, K), 80), _ints((N, K), 81)
    bias, resid = _ints((N,), 82) * 8, _ints((M, N), 83) * 16
    g = torch.Generator().manual_seed(84)
    a_map = torch.randint(0, R, (M,), generator=g).to(torch.int32)
    want = (a[a_map.long()] @ w.T + bias + resid).float().to(F16)
    x, wt, b, r = _h(a, dev), _h(w, dev), bias.float().to(dev), _h(resid, dev)
    assert torch.equal(ops.linear(x, wt, bias=b, resid=r, a_map=a_map.to(dev)).cpu(), want)
    xr = r.clone()
    ops.linear(x, wt, bias=b, resid=xr, a_map=a_map.to(dev), out=xr)
    assert torch.equal(xr.cpu(), want)


@pytest.mark.parametrize("M,N,K,gather", [(2048, 1280, 1280, False), (1024, 1280, 5120, False), (1536, 1280, 1280, True)])
def test_f16_linear_rowstats(dev, M, N, K, gather):
    """haff_gemm_f16_rowstats (SAM proj / lin2 + the next LayerNorm's statistics), with the a_map gather that brings window rows
    back: output == exact, in place on the residual; statistics == row_stats of the f16 rows written."""
    ops = _ops()
    R = M + 100 if gather else M
    a, w = _ints((R, K), 90), _ints((N, K), 91)
    bias, resid = _ints((N,), 92) * 8, _ints((M, N), 93) * 16
    a_map = None
    rows = a
    if gather:
        g = torch.Generator().manual_seed(94)
        a_map = torch.randperm(R, generator=g)[:M].to(torch.int32)
        rows = a[a_map.long()]
    want = (rows @ w.T + bias + resid).float().to(F16)
    r = _h(resid, dev)
    out, st = ops.linear_rowstats(_h(a, dev), _h(w, dev), bias.float().to(dev), r, 1e-6, out=r,
                                  a_map=None if a_map is None else a_map.to(dev))
    assert torch.equal(out.cpu(), want)
    exp = ops.row_stats(out, 1e-6)
    assert (st[:, 0] - exp[:, 0]).abs().max().item() <= 1e-4 * exp[:, 0].abs().max().item() + 1e-5
    assert ((st[:, 1] - exp[:, 1]).abs() / exp[:, 1]).max().item() <= 1e-4


@pytest.mark.parametrize("ratio", [30.0, 100.0])
def test_f16_linear_rowstats_with_a_large_row_mean(dev, ratio):
    """Rows whose mean is `ratio` x their spread: the producer's statistics must not cancel catastrophically (fp16 rows)."""
    ops = _ops()
    M, N, K = 512, 1280, 256
    a, w = _ints((M, K), 95), _ints((N, K), 96)
    exact = a @ w.T
    spread = exact.std().item()
    bias = torch.full((N,), float(round(ratio * spread)))
    resid = torch.zeros((M, N))
    out, st = ops.linear_rowstats(_h(a, dev), _h(w, dev), bias.to(dev), _h(resid, dev), 1e-6)
    assert torch.equal(out.cpu(), (exact + bias.double()).float().to(F16))
    of = out.double()
    mean, rstd = of.mean(-1), torch.rsqrt(of.var(-1, unbiased=False) + 1e-6)
    mean_rel = ((st[:, 0].double() - mean).abs() / mean.abs()).max().item()
    rstd_rel = ((st[:, 1].double() - rstd).abs() / rstd).max().item()
    print(f"mean / spread = {ratio:g}: mean rel err {mean_rel:.2e}, rstd rel err {rstd_rel:.2e}")
    assert mean_rel <= 5e-5   # measured 2.1e-5 (ratio 30), 1.8e-5 (100)
    assert rstd_rel <= 1.5e-6 * ratio * ratio + 5e-6   # half the bf16 test's bound


# --- weight-streaming kernel, split-K, row tail -------------------------------------------------------------------------------

@pytest.mark.parametrize("M", [1, 8, 16, 17, 31, 32, 33, 64])
@pytest.mark.parametrize("N,K", [(4096, 4096), (1024, 11008), (998, 384)])
def test_f16_gemm_skinny(dev, M, N, K):
    """gemm_skinny_kernel<MT, ..., F16> across its MT boundaries (16 / 17, 32 / 33), with the workspace (haff_gemm_f16_ws: the
    split-K skinny form and the split-K tile path) and without (haff_gemm_f16): exact with bias + residual, plain exact."""
    ops = _ops()
    import haff.ops as hops
    a, w = _ints((M, K), M), _ints((N, K), N)
    bias, resid = _ints((N,), 3) * 8, _ints((M, N), 4) * 16
    exact = a @ w.T
    x, wt = _h(a, dev), _h(w, dev)
    got = ops.linear(x, wt, bias=bias.float().to(dev), resid=_h(resid, dev))
    assert torch.equal(got.cpu(), (exact + bias + resid).float().to(F16))
    lib = hops.load_library()
    for out_f32 in (0, 1):
        out = torch.empty((M, N), dtype=torch.float32 if out_f32 else F16, device=dev)
        rc = lib.haff_gemm_f16(x.data_ptr(), K, wt.data_ptr(), K, out.data_ptr(), N, None, None, 0, None, M, N, K, 0, out_f32, 0,
                               hops._stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(out.cpu(), exact.float().to(out.dtype)), out_f32


@pytest.mark.parametrize("M", [8, 16])
@pytest.mark.parametrize("N", [351, 2808])
@pytest.mark.parametrize("K", [22016, 27648])
def test_f16_gemm_skinny_rank_products(dev, M, N, K):
    """The f16 LoRA nodes' rank products (8 / 16 rank rows over K = 2F at 7B / 13B) into a strided [rows][roundup(N, 16)] view:
    exact integer operands, so the f16 (and f32) result EQUALS the exact sum rounded once; the pad columns stay untouched."""
    ops = _ops()
    a, w = _ints((M, K), 130 + M), _ints((N, K), 131)
    exact = a @ w.T
    ld = (N + 15) // 16 * 16
    for odt in (F16, torch.float32):
        buf = torch.full((M, ld), 3.0, dtype=odt, device=dev)
        ops.linear(_h(a, dev), _h(w, dev), out=buf[:, :N])
        assert torch.equal(buf[:, :N].cpu(), exact.float().to(odt)), odt
        assert (buf[:, N:] == 3.0).all()


@pytest.mark.parametrize("M,N,K", [(64, 22016, 4096), (40, 16384, 4096), (288, 22016, 4096), (100, 2048, 4096)])
def test_f16_gemm_split_k_swiglu(dev, M, N, K):
    """SwiGLU through the split-K tile path's skinny_reduce_kernel<true> (and the skinny kernel where the shape keeps it):
    silu(gate) * up of the exact sums, within one f16 ulp."""
    ops = _ops()
    a, w = _ints((M, K), 100), _ints((N, K), 101) * 2.0 ** -6
    got = ops.linear(_h(a, dev), _h(w, dev), swiglu=True)
    _within_ulp(got, _swiglu_ref(a @ w.T), f"swiglu {M}x{N}x{K}")


@pytest.mark.parametrize("M,N,K", [(288, 4096, 4096), (288, 4096, 11008), (257, 1003, 1024), (64, 4096, 11008)])
def test_f16_gemm_split_k_residual(dev, M, N, K):
    """Split-K with bias + GELU + residual (skinny_reduce_kernel<true>, uneven K slices at 11008): bias -> act -> +resid in fp32
    (plain exact, GELU within one ulp)."""
    ops = _ops()
    a, w = _ints((M, K), 110), _ints((N, K), 111)
    bias, resid = _ints((N,), 112) * 8, _ints((M, N), 113) * 16
    exact = a @ w.T + bias
    x, wt, b, r = _h(a, dev), _h(w, dev), bias.float().to(dev), _h(resid, dev)
    assert torch.equal(ops.linear(x, wt, bias=b, resid=r).cpu(), (exact + resid).float().to(F16))
    _within_gelu(ops.linear(x, wt, bias=b, act=1, resid=r), F.gelu(exact) + resid, "split-K gelu + residual")


@pytest.mark.parametrize("M,N,K,inplace", [(4136, 4096, 128, False), (16448, 1024, 256, True)])
def test_f16_linear_row_tail_split(dev, M, N, K, inplace):
    """linear()'s SPLIT_ROW_TAIL two-launch form in f16 (whole 256-row tiles + a weight-streaming tail): == the one-launch form
    and == exact, bias + in-place residual included."""
    ops = _ops()
    import haff.ops as hops
    a, w = _ints((M, K), 120), _ints((N, K), 121)
    bias, resid = _ints((N,), 122) * 8, _ints((M, N), 123) * 16
    want = (a @ w.T + bias + resid).float().to(F16)
    x, wt, b, r = _h(a, dev), _h(w, dev), bias.float().to(dev), _h(resid, dev)
    assert hops.SPLIT_ROW_TAIL
    o_split = r.clone() if inplace else None
    o_split = ops.linear(x, wt, bias=b, resid=o_split if inplace else r, out=o_split)
    hops.SPLIT_ROW_TAIL = False
    try:
        o_one = ops.linear(x, wt, bias=b, resid=r)
    finally:
        hops.SPLIT_ROW_TAIL = True
    assert torch.equal(o_split.cpu(), want) and torch.equal(o_one.cpu(), want)


@pytest.mark.parametrize("M,N,K", [(4400, 4100, 128), (8192, 2304, 320), (2100, 33000, 256)])
def test_f16_gemm_ring_loop_across_tiles(dev, M, N, K):
    """The persistent 8-wave tile looping over many tiles per workgroup (f16): exact."""
    ops = _ops()
    a, w = _ints((M, K), 130), _ints((N, K), 131)
    got = ops.linear(_h(a, dev), _h(w, dev))
    assert torch.equal(got.cpu(), (a @ w.T).float().to(F16))


@pytest.mark.parametrize("M", [1, 3, 8])
def test_f16_linear_rms_producer_ssq_out(dev, M):
    """haff_gemm_f16_rms: the residual product emits per-workgroup sums of squares of its f16 output (ssq_out), and the next
    product on norm-folded weights turns those partials into 1/rms — the producer's partials equal the sums over the f16 rows it
    wrote, its output equals the plain product, and the consumer equals RMSNorm + product."""
    ops = _ops()
    H, N2, eps = 4096, 12288, 1e-5
    a, wo = _ints((M, H), 140), _ints((H, H), 141)
    x0 = _ints((M, H), 142) * 16
    x1_exact = (a @ wo.T + x0).float().to(F16)
    g = torch.Generator().manual_seed(143)
    gamma = 1.0 + 0.3 * torch.randn((H,), generator=g)
    w2 = torch.randn((N2, H), generator=g) * H ** -0.5
    w2f = (w2 * gamma[None, :]).to(F16)
    parts = torch.full((H // 16, 16), float("nan"), device=dev)
    x1 = ops.linear_rms(_h(a, dev), _h(wo, dev), resid=_h(x0, dev), out=_h(x0, dev), ssq_out=parts)
    assert torch.equal(x1.cpu(), x1_exact)
    ssq = (x1_exact.double() ** 2).view(M, H // 16, 16).sum(-1).T
    assert ((parts[:, :M].double().cpu() - ssq).abs() <= 1e-6 * ssq + 1e-30).all()
    y = ops.linear_rms(x1, w2f.to(dev), ssq_in=parts, eps=eps)
    xd = x1_exact.double()
    ref = (xd * torch.rsqrt((xd ** 2).mean(-1, keepdim=True) + eps)) @ w2f.double().T
    err = (y.double().cpu() - ref).abs().max().item()
    print(f"rms consumer M={M}: max|err| {err:.3e} of {ref.abs().max().item():.3e}")
    assert err <= 9e-4 * ref.abs().max().item()   # measured 3.6e-4 (M = 3, 8)


# --- attention ------------------------------------------------------------------------------------------------------------

def _rand16(shape, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(F16)


def _relpos_ref(q, k, v, scale, th, tw, S):
    """fp64 attention with the decomposed rel-pos bias from f16-rounded tables; q/k/v [B,H,N,d] -> [B,N,H*d]"""
    B, H, N, d = q.shape
    qd = q.double()
    idx = torch.arange(S, device=q.device)[:, None] - torch.arange(S, device=q.device)[None, :] + (S - 1)
    thd, twd = th.to(F16).double(), tw.to(F16).double()
    q6 = qd.reshape(B, H, S, S, d)
    rh = torch.einsum("bhyxc,ykc->bhyxk", q6, thd[idx])
    rw = torch.einsum("bhyxc,xkc->bhyxk", q6, twd[idx])
    s = (qd @ k.double().transpose(-1, -2)) * scale + (rh[..., :, None] + rw[..., None, :]).reshape(B, H, N, N)
    o = torch.softmax(s, -1) @ v.double()
    return o.permute(0, 2, 1, 3).reshape(B, N, H * d)


def _check(got, ref, rel, what):
    err = (got.double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"{what}: max|err| {err:.3e} = {err / scale:.3e} of scale {scale:.3f}")
    assert torch.isfinite(got).all() and got.dtype == F16
    assert err <= rel * scale, (what, err, scale)


# window attention: measured max|err| / scale 5.5e-4 ... 6.2e-4 on MI355X; the bound is 1.5e-3 (the bf16 tests: 2e-2)

def test_f16_window_attention_pad_token(dev):
    """haff_window_attention_f16 with grid = 20, pad_token: the padded tokens' rows are never written (NaN here) and the kernel
    takes the pad token row instead: == the same windows with the pad rows filled in, bit for bit."""
    ops = _ops()
    S, d, H, grid, nimg = 14, 80, 2, 20, 2
    N, wps = S * S, 2
    n_win = nimg * wps * wps
    qkv = (_rand16((n_win * N + 1, 3, H, d), 48, 1.5)).to(dev)
    pad_tok = qkv[-1].clone()
    is_pad = torch.zeros((n_win, S, S), dtype=torch.bool, device=dev)
    for w in range(n_win):
        wy, wx = (w % 4) // 2, (w % 4) % 2
        is_pad[w, max(0, grid - wy * S):, :] = True
        is_pad[w, :, max(0, grid - wx * S):] = True
    full = qkv[:-1].view(n_win, N, 3, H, d).clone()
    full[is_pad.view(n_win, N)] = pad_tok
    holes = qkv.clone()
    holes[:-1].view(n_win, N, 3, H, d)[is_pad.view(n_win, N)] = float("nan")
    th = (torch.randn((2 * S - 1, d)) * 0.5).to(dev)
    tw = (torch.randn((2 * S - 1, d)) * 0.5).to(dev)

    def views(buf):
        q5 = buf.view(n_win, N, 3, H, d)
        return (q5[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    q, k, v = views(holes[:-1])
    got = ops.window_attention(q, k, v, d ** -0.5, th, tw, S, grid=grid, pad_token=n_win * N)
    qf, kf, vf = views(full)
    ref = ops.window_attention(qf, kf, vf, d ** -0.5, th, tw, S)
    real = ~is_pad.view(n_win, N)
    assert torch.isfinite(got[real]).all()
    assert torch.equal(got[real], ref[real])
    _check(ref, _relpos_ref(qf, kf, vf, d ** -0.5, th, tw, S), 1.5e-3, "window f16 padded windows vs fp64")


@pytest.mark.parametrize("n_win", [5, 8, 48])
def test_f16_window_attention_fused(dev, n_win):
    """haff_window_attention_f16 on the ViT-H window geometry (16 heads, both grid -> workgroup mappings) vs fp64."""
    ops = _ops()
    S, d, H = 14, 80, 16
    N = S * S
    qkv = _rand16((n_win, N, 3, H, d), 45, 1.5).to(dev)
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    th = (torch.randn((2 * S - 1, d)) * 0.5).to(dev)
    tw = (torch.randn((2 * S - 1, d)) * 0.5).to(dev)
    got = ops.window_attention(q, k, v, d ** -0.5, th, tw, S)
    _check(got, _relpos_ref(q, k, v, d ** -0.5, th, tw, S), 1.5e-3, f"window f16 n_win={n_win}")


def test_f16_global_attention_16_heads_two_frames(dev):
    """haff_global_attention_f16 as the product runs it: 16 heads x 2 frames, N = 4096, vs fp64 (per frame). Tables of 0.25 make
    rel-pos biases that put later key tiles more than 16 log2 units above the first one: attn_global_pp_kernel's lazy softmax
    reference must move before p = 2^(s - m_run) leaves the f16 range (with the bf16 threshold of 40 the output was NaN)."""
    ops = _ops()
    S, d, H, B = 64, 80, 16, 2
    N = S * S
    qkv = _rand16((B, N, 3, H, d), 80).to(dev)
    q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    th = _rand16((2 * S - 1, d), 81, 0.25).float().to(dev)
    tw = _rand16((2 * S - 1, d), 82, 0.25).float().to(dev)
    assert ops.global_attention_supported(q, k, v, S)
    got = ops.global_attention(q, k, v, d ** -0.5, th, tw, S)
    assert torch.equal(got, ops.global_attention(q, k, v, d ** -0.5, th, tw, S)), "repeat launch differs"
    for b in range(B):
        for h0 in range(0, H, 8):
            hs = slice(h0, h0 + 8)
            ref = _relpos_ref(q[b:b + 1, hs], k[b:b + 1, hs], v[b:b + 1, hs], d ** -0.5, th, tw, S)
            _check(got[b:b + 1].view(1, N, H, d)[:, :, hs].reshape(1, N, 8 * d), ref, 4e-3, f"global f16 frame {b} heads {h0}+")


def test_f16_global_attention_score_jump_beyond_first_tile(dev):
    """Scores of later key tiles 12 (17.3 log2 units) above every score of the first tile, no rel-pos: the fused global kernel
    (haff_global_attention_f16) and the two-kernel path (rel-pos tables + haff_attention_f16, the same pp kernel) stay finite and
    match fp64. The lazy reference moves at 15 log2 units in f16; without that p reached 2^17 = inf."""
    ops = _ops()
    S, d, H, B = 64, 80, 2, 1
    N = S * S
    scale = d ** -0.5
    q = _rand16((B, H, N, d), 90, 0.5).double()
    q[..., 0] = 1.0
    k = _rand16((B, H, N, d), 91, 0.5).double()
    k[..., 0] = 0.0
    k[:, :, S:, 0] = 12.0 / scale            # every key outside the first tile (grid row 0) gets +12 on the score
    v = _rand16((B, H, N, d), 92).double()
    qkv = torch.stack([q, k, v], 2).to(F16).to(dev).permute(0, 3, 2, 1, 4).contiguous()
    qd, kd, vd = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    zeros = torch.zeros((2 * S - 1, d), device=dev)
    ref = _relpos_ref(qd, kd, vd, scale, zeros, zeros, S)
    got = ops.global_attention(qd, kd, vd, scale, zeros, zeros, S)
    _check(got, ref, 4e-3, "global f16, score jump after the first tile")
    rh, rw = ops.relpos_tables(qd, zeros, zeros, S)
    _check(ops.attention(qd, kd, vd, scale, relh=rh, relw=rw, S=S), ref, 4e-3, "two-kernel global f16, score jump")


# --- elementwise kernels ----------------------------------------------------------------------------------------------------

def test_f16_rope_cache_against_torch(dev):
    """haff_rope_cache / haff_rope_cache_rows (dtype 3) against RoPE written out in fp64 on the same f16 rows: q and k rotated,
    v copied, the cache rows written at pos0 (per row for the ragged form)."""
    ops = _ops()
    B, T, H, d, Tmax = 3, 37, 4, 128, 64
    inv = 1.0 / (10000.0 ** (torch.arange(0, d, 2, dtype=torch.float64) / d))
    ang = torch.arange(Tmax, dtype=torch.float64)[:, None] * inv[None, :]
    cs = torch.cat([torch.cos(ang), torch.sin(ang)], 1).float()
    qkv = _rand16((B * T, 3 * H * d), 150, 2.0)

    def rot(x, pos):   # x [B, T, H, d] (rotate_half form), pos [B, T]
        c, s = cs[pos, :d // 2].double(), cs[pos, d // 2:].double()
        c, s = torch.cat([c, c], -1)[:, :, None], torch.cat([s, s], -1)[:, :, None]
        x = x.double()
        xr = torch.cat([-x[..., d // 2:], x[..., :d // 2]], -1)
        return x * c + xr * s
    for rows in (False, True):
        pos0 = torch.tensor([5, 0, 20]) if rows else torch.tensor([9, 9, 9])
        pos = pos0[:, None] + torch.arange(T)[None, :]
        t = qkv.view(B, T, 3, H, d)
        q_ref, k_ref = rot(t[:, :, 0], pos), rot(t[:, :, 1], pos)
        buf = qkv.clone().to(dev)
        kc = torch.zeros((B, Tmax, H * d), dtype=F16, device=dev)
        vc = torch.zeros_like(kc)
        if rows:
            ops.rope_cache_rows(buf, kc, vc, cs.to(dev), B, T, H, H, d, pos0.to(torch.int32).to(dev))
        else:
            ops.rope_cache(buf, kc, vc, cs.to(dev), B, T, H, H, d, 9)
        qg = buf.view(B, T, 3, H, d)[:, :, 0].cpu()
        for b in range(B):
            p = int(pos0[b])
            kg = kc[b, p:p + T].view(T, H, d).cpu()
            _within_ulp(kg, k_ref[b], f"rope k rows={rows}", 1e-6)
            assert torch.equal(vc[b, p:p + T].cpu(), t[b, :, 2].reshape(T, H * d))
            assert (kc[b, :p] == 0).all() and (kc[b, p + T:] == 0).all()
        _within_ulp(qg, q_ref, f"rope q rows={rows}", 1e-6)


def test_f16_embed_splice_softmax_im2col_patchify(dev):
    """embed_splice, softmax_rows, im2col3x3 and patchify_nchw on f16 rows against plain torch."""
    ops = _ops()
    # embed_splice: one image block spliced at the image token of every sequence
    B, L, Hd, V, n_img = 2, 9, 256, 50, 5
    embed = _rand16((V, Hd), 160).to(dev)
    img = _rand16((B, n_img, Hd), 161).to(dev)
    g = torch.Generator().manual_seed(162)
    ids = torch.randint(0, V, (B, L), generator=g)
    img_pos = torch.tensor([2, 6], dtype=torch.int32)
    ids[torch.arange(B), img_pos.long()] = -200
    got = ops.embed_splice(ids.to(dev), img_pos.to(dev), embed, img).cpu()
    for b in range(B):
        p = int(img_pos[b])
        exp = torch.cat([embed.cpu()[ids[b, :p]], img.cpu()[b], embed.cpu()[ids[b, p + 1:]]])
        assert torch.equal(got[b], exp)
    # softmax_rows of f16 rows (fp32 out)
    x = _rand16((37, 1000), 163, 4.0).to(dev)
    sm = ops.softmax_rows(x)
    ref = torch.softmax(x.double(), -1)
    assert sm.dtype == torch.float32 and (sm.double() - ref).abs().max().item() <= 5.5e-6   # measured 2.3e-6
    # im2col3x3 of an f16 NHWC map: column block (dy, dx) of pixel (y, x) holds x[y+dy-1, x+dx-1] (zero outside)
    Bi, Hi, Wi, C = 2, 9, 7, 16
    xm = _rand16((Bi, Hi, Wi, C), 164).to(dev)
    cols = ops.im2col3x3(xm).cpu().view(Bi, Hi, Wi, 9, C)
    pad = F.pad(xm.cpu().permute(0, 3, 1, 2).float(), (1, 1, 1, 1)).permute(0, 2, 3, 1)
    for dy in range(3):
        for dx in range(3):
            assert torch.equal(cols[:, :, :, dy * 3 + dx].float(), pad[:, dy:dy + Hi, dx:dx + Wi])
    # patchify_nchw to f16 patches, K padded: row (b, gy, gx), column c * P * P + py * P + px
    P, gh, gw = 4, 3, 5
    Kp = 3 * P * P + 16
    xi = torch.randn((2, 3, gh * P, gw * P), generator=g).to(dev)
    pt = ops.patchify_nchw(xi, P, gh, gw, Kp, F16).cpu()
    ref = xi.cpu().view(2, 3, gh, P, gw, P).permute(0, 2, 4, 1, 3, 5).reshape(2 * gh * gw, 3 * P * P)
    assert torch.equal(pt[:, :3 * P * P], ref.to(F16)) and pt[:, 3 * P * P:].abs().max().item() == 0
