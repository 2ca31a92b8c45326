"""Every launch variant of the NF4 and int8 products against the CPU restatements, at the shapes that pick each one.

haff_gemm_nf4_f16 and the weight-streaming int8 form are instantiated per activation tile count MT (M <= 16, <= 32, <= 64), per
weight tiles per workgroup NT (two 16-row tiles when that still leaves >= 192 workgroups, else one) and per SwiGLU; the tiled int8
form with and without SwiGLU. Each is compared here with a plain reference of the same operation:
- NF4: nf4_ref.product (float64 on the dequantised weights) within nf4_ref.tol, on every row and on sampled columns that always
  include the first and last column of the edge tiles, the last tile and column N - 1;
- int8: int8_ref (quantize_rows + product + epilogue) bit for bit, or within an fp32 ulp budget of the transcendental epilogues;
- the activation quantiser's one-launch row kernel (seg_rows = 1) bit for bit: CA, SCA, the sticky masks, the column lists;
- the model's own non-Llama int8 calls (mm_projector, text_hidden_fcs, lm_head) and LlamaHip._lin's NF4 dispatch at M = 64 / 65
  with its lazily grown dequantisation scratch.

Instantiation -> a test that compares it with the reference ([M-N] ids; MT = 1 has no two-tile form without SwiGLU):
  gemm_nf4_kernel       MT=1 NT=1                test_nf4_mt_and_nt_forms[16-4096]
                        MT=2 NT=1 / NT=2         test_nf4_mt_and_nt_forms[17-6128] / [32-6144]
                        MT=4 NT=1 / NT=2         test_nf4_mt_and_nt_forms[33-6128] / [64-32003]
                        MT=1 / 2 / 4 SwiGLU      test_nf4_swiglu[1-shape0] / [17-shape0] / [64-shape1]
  gemm_i8_skinny_kernel MT=1 NT=1                test_int8_forms_m_and_n[skinny-16-4096]
                        MT=2 NT=1 / NT=2         test_int8_forms_m_and_n[skinny-17-6128] / [skinny-24-6144]
                        MT=4 NT=1 / NT=2         test_int8_forms_m_and_n[skinny-33-4160] / [skinny-64-32003]
                        MT=1 / 2 / 4 SwiGLU      test_int8_swiglu[1-shape0] / [17-shape0] / [64-shape1]  (both forms)
  gemm_i8_tiled_kernel  plain / SwiGLU           test_int8_tiled_large_m[129-4160] / test_int8_swiglu[129-shape0]
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/int8_ref.py, tests/nf4_ref.py
import int8_ref as IR   # noqa: E402
import nf4_ref as NR   # noqa: E402

pytestmark = pytest.mark.gpu

M_SKINNY = [1, 16, 17, 24, 32, 33, 48, 64]       # every MT and both sides of each of its boundaries
N_FORMS = [4096, 6128, 6144, 12288, 32003]       # NT = 1; the tiles / 2 >= 192 switch (383 / 384 tiles); NT = 2; odd tile count
SLOPE = 1.13                                     # max |act'| of GELU (1.129), SiLU / quick-GELU (1.100) and ReLU (1)


def _cols(n_out, seed, n_rand=160):
    """Sampled output columns: first and last column of the first four and the last three 16-column tiles, N - 1, random others."""
    tiles = (n_out + 15) // 16
    c = {n_out - 1}
    for t in sorted({0, 1, 2, 3, tiles - 3, tiles - 2, tiles - 1}):
        if 0 <= t < tiles:
            c.update((16 * t, min(16 * t + 15, n_out - 1)))
    c.update(np.random.default_rng(seed).choice(n_out, min(n_rand, n_out), replace=False).tolist())
    return np.array(sorted(c))


def _gate_up(cols):
    """Weight rows of SwiGLU output columns in the [gate x16 | up x16] interleave: (gate rows, up rows)."""
    g = 32 * (cols // 16) + cols % 16
    return g, g + 16


def _act64(t, act):
    if act == IR.ACT_NONE:
        return t
    if act == IR.ACT_RELU:
        return t.clamp_min(0)
    if act == IR.ACT_GELU:
        return 0.5 * t * (1 + torch.erf(t * 0.7071067811865476))
    if act == IR.ACT_QUICK_GELU:
        return t * torch.sigmoid(1.702 * t)
    return t * torch.sigmoid(t)


def _act_err(x, v):
    """Bound of the device's own fp32 evaluation error of an activation (erff / __expf / rcpf, a few ulps, and the exponent's
    rounding growing with |x|) at input x, value v (float64 tensors)."""
    return 2.0 ** -20 * (x.abs() + 1) * v.abs() + 2.0 ** -22 * x.abs()


def _out_ulp(v, od):
    return v.abs().clamp_min(2.0 ** -14) * 2.0 ** -10 if od == torch.float16 else v.abs() * 2.0 ** -23


class _Out:
    """An output buffer with prior contents (the residual when it aliases C), optionally wider than n_out (ldc > n_out) and with more
    rows than M (a row map's target), and the row map: a permutation into M + 3 rows, every fifth row from row 2 on dropped (-1)."""

    def __init__(self, dev, M, n_out, od, row_map, wide, seed):
        g = torch.Generator().manual_seed(seed)
        self.R = M + 3 if row_map else M
        self.n_out = n_out
        self.prior = (torch.randn(self.R, n_out + (40 if wide else 0), generator=g)).to(od)
        self.buf = self.prior.to(dev, copy=True)
        self.rows = np.arange(M)
        self.map = None
        if row_map:
            self.rows = torch.randperm(self.R, generator=g)[:M].numpy()
            self.rows[2::5] = -1
            self.map = torch.from_numpy(self.rows.astype(np.int32)).to(dev)

    @property
    def out(self):
        return self.buf[:, :self.n_out]

    def fresh(self):
        self.buf = self.prior.to(self.buf.device, copy=True)

    def check_untouched(self):
        """Rows the map does not write and the columns beyond n_out: bit for bit the prior contents."""
        got = self.buf.cpu()
        keep = np.setdiff1d(np.arange(self.R), self.rows[self.rows >= 0])
        assert torch.equal(got[keep], self.prior[keep])
        assert torch.equal(got[:, self.n_out:], self.prior[:, self.n_out:])
        return got


# ---- NF4 -----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def _nf4_weight(dev, N, K):
    from haff import quant
    g = torch.Generator(device=dev).manual_seed(N * 131 + K)
    return quant.quantize([(torch.randn(N, K, device=dev, generator=g) * 0.02, None)], dev)


def _nf4_check(dev, M, N, K, swiglu=False, act=IR.ACT_NONE, bias=True, od=torch.float16, resid=False, row_map=False, wide=False,
               seed=0):
    """ops.linear_nf4 vs nf4_ref.product on every row and sampled columns; a second run must give the same bits. resid: the f16
    output's prior contents (aliasing C) or, for fp32 out, a separate fp32 tensor."""
    from haff import ops
    w = _nf4_weight(dev, N, K)
    g = torch.Generator().manual_seed(seed * 1000 + M)
    lda = K + 64 if wide else K
    xfull = torch.randn(M, lda, generator=g).half()
    x, xd = xfull[:, :K], xfull.to(dev)[:, :K]
    b = torch.randn(N, generator=g) * 0.5 if bias else None
    n_out = N // 2 if swiglu else N
    o = _Out(dev, M, n_out, od, row_map, wide, seed + M)
    r32 = torch.randn(o.R, n_out, generator=g) if resid and od == torch.float32 else None
    bd = None if b is None else b.to(dev)

    def run():
        rs = None
        if resid:
            rs = o.out if od == torch.float16 else r32.to(dev)
        ops.linear_nf4(xd, w.packed, w.absmax, bias=bd, act=act, resid=rs, row_map=o.map, out=o.out, swiglu=swiglu)
        return o.check_untouched()
    got = run()
    o.fresh()
    again = run()
    assert torch.equal(got, again)                       # repeat runs bitwise equal
    cols = _cols(n_out, seed + M)
    wrows = np.concatenate(_gate_up(cols)) if swiglu else cols
    wr = torch.from_numpy(wrows)
    pk, am = w.packed[wr.to(dev)].cpu(), w.absmax[wr.to(dev)].cpu()
    bb = None if b is None else b[wr]
    pre = NR.product(x, pk, am, bb)
    tpre = NR.tol(x, NR.dequant(pk, am), bb, od)         # accumulation only
    if swiglu:
        n = len(cols)
        gt, ut, tg, tu = pre[:, :n], pre[:, n:], tpre[:, :n], tpre[:, n:]
        sg = gt * torch.sigmoid(gt)
        v = sg * ut
        t = SLOPE * ut.abs() * tg + sg.abs() * tu + _act_err(gt, v)
    else:
        v = _act64(pre, act)
        t = (SLOPE if act != IR.ACT_NONE else 1.0) * tpre + (_act_err(pre, v) if act not in IR.EXACT_ACTS else 0)
    rows = o.rows
    w_rows = rows >= 0
    base = (o.prior if r32 is None else r32)[rows[w_rows]][:, cols].double() if resid else 0
    ref = v[w_rows] + base
    t = t[w_rows] + _out_ulp(ref, od)
    d = (got[rows[w_rows]][:, cols].double() - ref).abs()
    bad = d > t
    assert not bad.any(), (M, N, K, int(bad.sum()), (d / t).max().item())


@pytest.mark.parametrize("N", N_FORMS)
@pytest.mark.parametrize("M", M_SKINNY)
def test_nf4_mt_and_nt_forms(dev, M, N):
    _nf4_check(dev, M, N, 4096, od=torch.float32 if N == 32003 else torch.float16)


@pytest.mark.parametrize("shape", [(2 * 11008, 4096), (2 * 13824, 5120), (64, 192)])
@pytest.mark.parametrize("M", [1, 16, 17, 32, 33, 64])
def test_nf4_swiglu(dev, M, shape):
    _nf4_check(dev, M, shape[0], shape[1], swiglu=True)


@pytest.mark.parametrize("K", [64, 192, 1024, 11008, 13824])
@pytest.mark.parametrize("M", [1, 17, 33])
def test_nf4_k_blocks(dev, M, K):
    """One 64-block (7 of the 8 waves empty), block counts that do not divide over 8 waves, the 7B / 13B down projections."""
    N = {11008: 4096, 13824: 5120}.get(K, 6144)
    _nf4_check(dev, M, N, K)


EPILOGUES = {
    "gelu": dict(act=IR.ACT_GELU), "quick_gelu": dict(act=IR.ACT_QUICK_GELU), "relu": dict(act=IR.ACT_RELU),
    "silu": dict(act=IR.ACT_SILU), "silu_f32": dict(act=IR.ACT_SILU, od=torch.float32), "no_bias": dict(bias=False),
    "resid_f16_alias": dict(resid=True), "resid_f32": dict(resid=True, od=torch.float32),
    "row_map_resid": dict(row_map=True, resid=True), "strided": dict(wide=True),
    "swiglu_row_map_strided": dict(swiglu=True, row_map=True, wide=True),
    "relu_f32_row_map_strided": dict(act=IR.ACT_RELU, od=torch.float32, row_map=True, wide=True, resid=True),
}


@pytest.mark.parametrize("variant", list(EPILOGUES))
@pytest.mark.parametrize("M", [1, 24, 64])
def test_nf4_epilogues(dev, M, variant):
    _nf4_check(dev, M, 6144, 4096, seed=3, **EPILOGUES[variant])


def test_nf4_lin_dispatch_boundary_and_scratch_growth(dev):
    """LlamaHip._lin at 7B width: M = 64 streams the NF4 weight, M = 65 dequantises it into the shared scratch and runs the f16
    product; then weights of other sizes through the same scratch: o (fits), down (K = 11008, fits), a 32000-row lm_head (grows
    it), o and down again. Every product within nf4_ref's tolerance of the float64 product."""
    from haff import config as hcfg
    from haff import quant
    from haff.llava import LlamaHip
    lc = hcfg.haff_7b().llm
    lc.layers = 0
    H, F = lc.hidden, lc.ffn
    sd = {"model.embed_tokens.weight": torch.zeros(8, H), "model.norm.weight": torch.ones(H),
          "lm_head.weight": torch.randn(64, H, generator=torch.Generator().manual_seed(1)) * 0.02}
    g = torch.Generator(device=dev).manual_seed(7)
    ws = {name: quant.quantize([(torch.randn(n, k, device=dev, generator=g) * 0.02, None)], dev)
          for name, (n, k) in {"qkv": (3 * H, H), "o": (H, H), "down": (H, F), "lm": (32000, H)}.items()}

    def check(m, name, M, seed):
        w = ws[name]
        N, K = w.shape
        x = torch.randn(M, K, generator=torch.Generator().manual_seed(seed)).half()
        got = m._lin(x.to(dev), w).cpu()
        cols = _cols(N, seed)
        ci = torch.from_numpy(cols).to(dev)
        pk, am = w.packed[ci].cpu(), w.absmax[ci].cpu()
        ref = NR.product(x, pk, am)
        t = NR.tol(x, NR.dequant(pk, am), None, torch.float16, ref)
        d = (got[:, cols].double() - ref).abs()
        assert (d <= t).all(), (name, M, (d / t).max().item())

    m = LlamaHip(sd, lc, torch.float16, dev, nf4=True)
    check(m, "qkv", 64, 1)
    assert m._scratch is None                            # the streamed product touches no scratch
    check(m, "qkv", 65, 2)
    m = LlamaHip(sd, lc, torch.float16, dev, nf4=True)
    sizes = []
    for i, name in enumerate(("o", "down", "lm", "o", "down")):
        check(m, name, 65, 10 + i)
        sizes.append(m._scratch.numel())
    assert sizes[0] == sizes[1] < sizes[2] == sizes[3] == sizes[4] == 32000 * H


# ---- int8 ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=8)
def _i8_weight(dev, N, K):
    """(f16 weight on the device, its Int8Weight)"""
    from haff import quant
    g = torch.Generator(device=dev).manual_seed(N * 17 + K)
    w = (torch.randn(N, K, device=dev, generator=g) * 0.02).half()
    return w, quant.quantize_int8([(w, None)], dev)


def _rows(M, K, seed, planted=(), lda=None):
    """f16 rows [M, lda or K] (take [:, :K] for a strided view): outlier feature dims planted (|a| >= 6 in most rows, always in
    row 0)."""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, lda or K, generator=g)
    for c in planted:
        a[:, c] *= 9.0
        a[0, c] = 7.5
    return a.half()


def _interleave(gt, ut):
    """[M, n] gate and up columns -> the [gate x16 | up x16] layout int8_ref.epilogue(swiglu=True) reads (n padded to 16)."""
    M, n = gt.shape
    p = -n % 16
    gp, up = np.pad(gt, ((0, 0), (0, p))), np.pad(ut, ((0, 0), (0, p)))
    return np.stack([gp.reshape(M, -1, 16), up.reshape(M, -1, 16)], axis=2).reshape(M, -1)


def _i8_check(dev, M, N, K, form=0, seg=None, thr=6.0, planted=(11, 1000), swiglu=False, act=IR.ACT_NONE, bias=True,
              od=torch.float16, resid=False, row_map=False, wide=False, seed=0, n_rand=160):
    """ops.int8_quantize_act + ops.linear_int8 vs int8_ref (quantize_rows + product + epilogue) on every row and sampled columns."""
    from haff import ops
    wdev, qw = _i8_weight(dev, N, K)
    seg = M if seg is None else seg
    afull = _rows(M, K, seed * 1000 + M, planted, lda=K + 64 if wide else None)
    a, ad = afull[:, :K], afull.to(dev)[:, :K]
    g = torch.Generator().manual_seed(seed + 1)
    b = torch.randn(N, generator=g) if bias else None
    n_out = N // 2 if swiglu else N
    o = _Out(dev, M, n_out, od, row_map, wide, seed + M)
    r32 = torch.randn(o.R, n_out, generator=g) if resid and od == torch.float32 else None
    q = ops.int8_quantize_act(ad, thr, seg)
    rs = None
    if resid:
        rs = o.out if od == torch.float16 else r32.to(dev)
    ops.linear_int8(q, qw.cb, qw.scb, bias=None if b is None else b.to(dev), act=act, resid=rs, row_map=o.map, out=o.out,
                    swiglu=swiglu, form=form)
    got = o.check_untouched()
    cols = _cols(n_out, seed + M, n_rand)
    wrows = np.concatenate(_gate_up(cols)) if swiglu else cols
    rcb, rscb = IR.quantize_weight(wdev[torch.from_numpy(wrows).to(dev)].float().cpu().numpy())
    an = a.float().numpy()
    rca, rsca, rmasks = IR.quantize_rows(an, thr, seg)
    y = IR.product(an, rca, rsca, rcb, rscb, rmasks, seg, None if b is None else b.numpy()[wrows])
    n, pad = len(cols), 0
    if swiglu:
        y = _interleave(y[:, :n], y[:, n:])
        pad = y.shape[1] // 2 - n
    prior = np.pad(o.prior[:, cols].numpy(), ((0, 0), (0, pad)))
    res = None if not resid else (prior if r32 is None else np.pad(r32[:, cols].numpy(), ((0, 0), (0, pad))))
    ref = IR.epilogue(y, act, res, od == torch.float32, None if o.map is None else o.rows, swiglu, out=prior)[:, :n]
    gc = got[:, cols].numpy()
    if act in IR.EXACT_ACTS and not swiglu:
        assert np.array_equal(gc.view(np.int16 if od == torch.float16 else np.int32),
                              ref.view(np.int16 if od == torch.float16 else np.int32)), (M, N, K, form, int((gc != ref).sum()))
    else:
        if swiglu:
            gt, ut = [torch.from_numpy(h.astype(np.float64))[:, :n] for h in IR.swiglu_split(y)]
            xin, v = gt, gt * torch.sigmoid(gt) * ut
        else:
            xin = torch.from_numpy(y.astype(np.float64))
            v = _act64(xin, act)
        rr = torch.from_numpy(ref.astype(np.float64))
        t = torch.zeros_like(rr)
        wr = o.rows >= 0
        t[o.rows[wr]] = _act_err(xin[wr], v[wr]) + _out_ulp(rr[o.rows[wr]], od)
        d = (torch.from_numpy(gc.astype(np.float64)) - rr).abs()
        assert (d <= t).all(), (M, N, K, form, (d / t.clamp_min(1e-30)).max().item())
    return int(rmasks.sum())


@pytest.mark.parametrize("N", [4096, 4096 + 64, 6128, 6144, 12288, 32003])
@pytest.mark.parametrize("M", [1, 16, 17, 24, 32, 33, 64])
@pytest.mark.parametrize("form", ["skinny", "tiled"])
def test_int8_forms_m_and_n(dev, form, M, N):
    from haff import ops
    f = ops.INT8_SKINNY if form == "skinny" else ops.INT8_TILED
    n = _i8_check(dev, M, N, 4096, f, seg=min(M, 16), planted=(11, 1000, 4095), seed=1)
    assert n > 0


@pytest.mark.parametrize("N", [4096, 4096 + 64, 6128, 6144, 12288, 32003])
@pytest.mark.parametrize("M", [65, 127, 129, 300])
def test_int8_tiled_large_m(dev, M, N):
    from haff import ops
    _i8_check(dev, M, N, 4096, ops.INT8_TILED, seg=100, planted=(5, 2222), seed=2)


@pytest.mark.parametrize("shape", [(2 * 11008, 4096), (2 * 13824, 5120), (64, 192)])
@pytest.mark.parametrize("M", [1, 17, 33, 64, 129])
def test_int8_swiglu(dev, M, shape):
    from haff import ops
    forms = [ops.INT8_TILED] if M > 64 else [ops.INT8_SKINNY, ops.INT8_TILED]
    for f in forms:
        _i8_check(dev, M, shape[0], shape[1], f, seg=min(M, 8), planted=(3, 77), swiglu=True, seed=4)


@pytest.mark.parametrize("variant", list(EPILOGUES))
@pytest.mark.parametrize("M", [1, 24, 64, 129])
def test_int8_epilogues(dev, M, variant):
    from haff import ops
    forms = [ops.INT8_TILED] if M > 64 else [ops.INT8_SKINNY, ops.INT8_TILED]
    for f in forms:
        _i8_check(dev, M, 6144, 4096, f, seg=min(M, 8), seed=5, **EPILOGUES[variant])


@pytest.mark.parametrize("N", [4096, 5120])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_int8_mm_projector(dev, B, N):
    """The projector's call: K = 1024 CLIP features, one 256-row segment per frame, bias, f16 out (lisa.py encode_images)."""
    _i8_check(dev, B * 256, N, 1024, seg=256, planted=(17, 700), seed=6)


@pytest.mark.parametrize("H", [4096, 5120])
@pytest.mark.parametrize("B", [1, 3])
def test_int8_text_hidden_fcs(dev, B, H):
    """text_hidden_fcs as lisa.py runs them: every row of each frame, one segment of Th rows per frame whose first valid[b] rows
    count (outliers planted in a padding row must not become columns), fc0 N = K = H with ReLU, then fc2 N = 256 on fc0's output."""
    from haff import ops, quant
    Th = 300
    valid = [Th, 263, 291][:B]
    g = torch.Generator(device=dev).manual_seed(H)
    w0 = (torch.randn(H, H, device=dev, generator=g) * 0.02).half()
    w2 = (torch.randn(256, H, device=dev, generator=g) * 0.02).half()
    b0, b2 = [torch.randn(n, generator=torch.Generator().manual_seed(n)) for n in (H, 256)]
    q0, q2 = quant.quantize_int8([(w0, None)], dev), quant.quantize_int8([(w2, None)], dev)
    x = _rows(B * Th, H, 8, planted=(9, H - 33))
    if B > 1:
        x[Th + 280, 123] = 50.0          # a padding row of frame 1: not one of its columns
    vd = torch.tensor(valid, dtype=torch.int32, device=dev)
    q = ops.int8_quantize_act(x.to(dev), 6.0, Th, vd)
    h = ops.linear_int8(q, q0.cb, q0.scb, bias=b0.to(dev), act=ops.ACT_RELU)
    qh = ops.int8_quantize_act(h, 6.0, Th, vd)
    y = ops.linear_int8(qh, q2.cb, q2.scb, bias=b2.to(dev)).cpu().numpy()
    cols = _cols(H, 8)
    xn = x.float().numpy()
    rca, rsca, rmasks = IR.quantize_rows(xn, 6.0, Th, valid)
    if B > 1:
        assert not rmasks[1, 123] and np.array_equal(q.ncols.cpu().numpy(), rmasks.sum(1))
    rcb, rscb = IR.quantize_weight(w0[torch.from_numpy(cols).to(dev)].float().cpu().numpy())
    rh = IR.epilogue(IR.product(xn, rca, rsca, rcb, rscb, rmasks, Th, b0.numpy()[cols]), IR.ACT_RELU)
    hc = h.cpu().numpy()
    assert np.array_equal(hc[:, cols].view(np.int16), rh.view(np.int16))
    hn = hc.astype(np.float32)                           # fc2 on the (checked) device fc0 output, all 256 columns
    rca, rsca, rmasks = IR.quantize_rows(hn, 6.0, Th, valid)
    rcb, rscb = IR.quantize_weight(w2.float().cpu().numpy())
    ry = IR.product(hn, rca, rsca, rcb, rscb, rmasks, Th, b2.numpy())
    assert np.array_equal(y.view(np.int16), ry.view(np.int16))


@pytest.mark.parametrize("H", [4096, 5120])
@pytest.mark.parametrize("B", [1, 4, 17, 40])
def test_int8_lm_head(dev, B, H):
    """lm_head as next_token_logits runs it: one row per frame (seg_rows = 1) against masks preset by the frame's prefix rows, fp32
    out, N = 32001 (B = 17 and 40: MT = 2 and 4 with two weight tiles per workgroup)."""
    from haff import ops
    N, T = 32001, 20
    wdev, qw = _i8_weight(dev, N, H)
    prefix = _rows(B * T, H, 9, planted=(2, 3000))
    for b in range(B):
        prefix[b * T + (b % T), 100 + b] = -30.0         # a column of frame b only
    last = _rows(B, H, 10)
    last[B - 1, 4000] = 8.0                              # an outlier of the last row: joins its own mask
    mk = torch.zeros((B, H // 32), dtype=torch.int32, device=dev)
    ops.int8_quantize_act(prefix.to(dev), 6.0, T, masks=mk)
    q = ops.int8_quantize_act(last.to(dev), 6.0, 1, masks=mk)
    y = ops.linear_int8(q, qw.cb, qw.scb, out_dtype=torch.float32).cpu().numpy()
    rm = np.zeros((B, H), dtype=bool)
    IR.quantize_rows(prefix.float().numpy(), 6.0, T, masks=rm)
    ln = last.float().numpy()
    rca, rsca, rm = IR.quantize_rows(ln, 6.0, 1, masks=rm)
    cols = _cols(N, 10)
    rcb, rscb = IR.quantize_weight(wdev[torch.from_numpy(cols).to(dev)].float().cpu().numpy())
    ry = IR.epilogue(IR.product(ln, rca, rsca, rcb, rscb, rm, 1), out_f32=True)
    assert np.array_equal(y[:, cols].view(np.int32), ry.view(np.int32))
    words = mk.cpu().numpy().astype(np.uint32)
    bits = ((words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(B, H).astype(bool)
    assert np.array_equal(bits, rm) and rm[B - 1, 4000]


@pytest.mark.parametrize("K", [4096, 5120, 11008, 13824])
@pytest.mark.parametrize("case", ["zero_masks_thr6", "preset_masks_thr6", "preset_masks_thr0"])
def test_int8_activation_row_kernel(dev, case, K):
    """haff_int8_quantize_act_f16 with seg_rows = 1 (one launch per call: every decode step, lm_head): CA, SCA, the masks, the column
    lists and their counts bit for bit; valid 0 / 1 per row; threshold 0 ignores the masks it is given and leaves them alone."""
    from haff import ops
    M = 12
    thr = 0.0 if case.endswith("thr0") else 6.0
    a = _rows(M, K, K, planted=(3, K // 2, K - 1))
    a[2, 77] = 6.0                                       # exactly the threshold
    a[4] = 0.0                                           # all-zero row
    a[5, :] = -7.0                                       # all-outlier row
    a[7, 9] = 65504.0
    a[0, 10] = -12.0                                     # row 0 is always valid
    rng = np.random.default_rng(K)
    valid = rng.integers(0, 2, M).astype(np.int32)
    valid[[0, 5]] = 1, 0
    pre = np.zeros((M, K), dtype=bool) if case.startswith("zero") else rng.random((M, K)) < 0.003
    words = (pre.reshape(M, -1, 32).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32)
    mk = torch.from_numpy(words.view(np.int32).copy()).to(dev)
    q = ops.int8_quantize_act(a.to(dev), thr, 1, torch.from_numpy(valid).to(dev), mk)
    rmask = pre.copy()
    rca, rsca, rmask = IR.quantize_rows(a.float().numpy(), thr, 1, valid, None if thr == 0 else rmask)
    if thr == 0:
        rmask = np.zeros_like(pre)                       # no decomposition: no columns
    assert np.array_equal(q.ca.cpu().numpy(), rca)
    assert np.array_equal(q.sca.cpu().numpy().view(np.int32), rsca.view(np.int32))
    got_words = mk.cpu().numpy().view(np.uint32)
    got_bits = ((got_words[:, :, None] >> np.arange(32, dtype=np.uint32)) & 1).reshape(M, K).astype(bool)
    assert np.array_equal(got_bits, pre if thr == 0 else rmask)
    nc = q.ncols.cpu().numpy()
    assert np.array_equal(nc, rmask.sum(1))
    cl = q.cols.cpu().numpy()
    for m in range(M):
        assert np.array_equal(cl[m, :nc[m]], np.flatnonzero(rmask[m]))
    if thr > 0:
        assert np.array_equal(rmask[5], pre[5]) and rmask[0, 10]   # the invalid all-outlier row put no columns in
