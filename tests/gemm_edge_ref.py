"""Float64 restatement of the 16-bit GEMM family (csrc/gemm_bf16.hip) and operand builders whose exact result is known.

No GPU import: everything here is plain torch on whatever device its arguments live on (the CPU in test_gemm_edge_ref_cpu.py; in
test_gemm_edge_kernels_gpu.py the builders run on the CPU and the float64 references on the device). The restatement follows the documented order of ops.linear and
the layout rules of the GemmArgs comments; the builders return float64 tensors that the 16-bit format holds exactly and assert the
condition under which fp32 accumulation is exact in ANY order, so that the kernels can be compared with ==.
"""
import math

import torch

BF16, F16, F32, F64 = torch.bfloat16, torch.float16, torch.float32, torch.float64
NAN, INF = float("nan"), float("inf")
ACT_NONE, ACT_GELU, ACT_QUICK_GELU, ACT_RELU, ACT_SILU = 0, 1, 2, 3, 4
WS_BYTES = 64 << 20      # the workspace ops.linear hands over
BK = 64


# ------------------------------------------------------------------------------------------------------------- conversions
def to16(y64, dtype, exact=False):
    """torch's conversion of y64.float(): round-to-nearest-even, inf past the largest finite value. exact: the caller declares the
    float64 values fp32-exact (an fp32 epilogue can then produce them without a rounding of its own); asserted here."""
    y32 = y64.float()
    if exact:
        ok = (y32.double() == y64) | torch.isnan(y64)
        assert bool(ok.all()), "the case is declared exact but its float64 result is not an fp32 value"
    return y32.to(dtype)


def _bits32(y64):
    return y64.float().contiguous().view(torch.int32)


def trunc_bf16(y64):
    """the mistake: f32 -> bf16 by dropping the low 16 bits (round toward zero)"""
    b = _bits32(y64) & ~0xFFFF
    return b.view(F32).to(BF16)


def half_away_bf16(y64):
    """the mistake: f32 -> bf16 by adding 0x8000 and dropping the low 16 bits (ties away from zero)"""
    b = (_bits32(y64) + 0x8000) & ~0xFFFF
    return b.view(F32).to(BF16)


def is16(t, dtype):
    return bool((t.to(dtype).double() == t).all())


# ------------------------------------------------------------------------------------------------------------- the product
def act_ref(x, act, quick=1.702, tanh_gelu=False):
    if act == ACT_NONE:
        return x
    if act == ACT_GELU:
        if tanh_gelu:
            return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))
        return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))
    if act == ACT_QUICK_GELU:
        return x * torch.sigmoid(quick * x)
    if act == ACT_RELU:
        return torch.clamp_min(x, 0.0)
    if act == ACT_SILU:
        return x * torch.sigmoid(x)
    raise ValueError(act)


def pre_act_ref(a, w, bias=None, a_map=None, ln_stats=None, ln_colsum=None, acc=None):
    """gather -> product -> folded norm rstd * (acc - mean * colsum) -> + bias, float64 [M, N]. acc: the gathered product, where the
    caller has it already (several epilogues of one product)"""
    if acc is None:
        rows = a if a_map is None else a[a_map.long()]
        acc = rows @ w.T
    y = acc
    if ln_stats is not None:
        mean, rstd = ln_stats[:, 0:1], ln_stats[:, 1:2]
        if ln_colsum is not None:
            y = y - mean * ln_colsum[None, :]
        y = rstd * y
    if bias is not None:
        y = y + bias[None, :]
    return y


def swiglu_ref(y):
    """weight rows interleaved [gate x16 | up x16]: output column 16 j + i = silu(y[32 j + i]) * y[32 j + 16 + i]"""
    M, N = y.shape
    g = y.view(M, N // 32, 2, 16)
    return (act_ref(g[:, :, 0], ACT_SILU) * g[:, :, 1]).reshape(M, N // 2)


def scatter_ref(y, resid, row_map, out):
    """+ resid (indexed like the output) and the store through row_map (negative entries dropped) into a COPY of out"""
    M = y.shape[0]
    out = torch.zeros_like(y) if out is None else out.clone()
    if row_map is None:
        assert out.shape[0] == M
        out[:] = y if resid is None else y + resid
        return out
    rm = row_map.long()
    keep = rm >= 0
    dst = rm[keep]
    out[dst] = y[keep] if resid is None else y[keep] + resid[dst]
    return out


def gemm_ref(a, w, bias=None, act=ACT_NONE, resid=None, row_map=None, out=None, swiglu=False, a_map=None, ln_stats=None,
             ln_colsum=None, acc=None):
    """ops.linear in float64: gather a_map -> product -> folded norm -> + bias -> act (SwiGLU pairs: silu(gate) * up, no other
    activation) -> + resid -> scatter through row_map into a copy of the caller's pre-filled `out`."""
    y = pre_act_ref(a, w, bias, a_map, ln_stats, ln_colsum, acc)
    y = swiglu_ref(y) if swiglu else act_ref(y, act)
    return scatter_ref(y, resid, row_map, out)


def heads_ref(y, row_map, out_flat, d, heads, part_stride, head_stride):
    """HEAD-MAJOR scatter: product column part * heads * d + h * d + c of row m -> out_flat[part * part_stride + h * head_stride +
    row_map[m] * d + c]; negative rows dropped. Returns a copy of out_flat."""
    M, N = y.shape
    out = out_flat.clone()
    n = torch.arange(N, device=y.device)
    part, h, c = n // (heads * d), (n // d) % heads, n % d
    col = part * part_stride + h * head_stride + c
    rm = row_map.long()
    keep = rm >= 0
    idx = rm[keep][:, None] * d + col[None, :]
    out[idx.reshape(-1)] = y[keep].reshape(-1)
    return out


def rope_rotate(u, cs_rows):
    """rotate-half on [..., 128] with table rows [..., cos(0..63) | sin(0..63)]"""
    c, s = cs_rows[..., :64], cs_rows[..., 64:]
    u1, u2 = u[..., :64], u[..., 64:]
    return torch.cat([u1 * c - u2 * s, u2 * c + u1 * s], -1)


def qkv_rope_ref(a, w, cs, B, T, H, pos0, kcache, vcache):
    """q|k|v projection (w in LOGICAL row order) + rotate-half RoPE at position pos0 + t of product row m = b * T + t; rotated q
    [B*T, H*128]; rotated k and plain v into copies of the caches [B, Tmax, H*128] at row (b, pos0 + t)."""
    d = 128
    y = (a @ w.T).view(B, T, 3, H, d)
    rows = cs[pos0:pos0 + T][None, :, None, :]
    q = rope_rotate(y[:, :, 0], rows).reshape(B * T, H * d)
    k, v = kcache.clone(), vcache.clone()
    k[:, pos0:pos0 + T] = rope_rotate(y[:, :, 1], rows).reshape(B, T, H * d)
    v[:, pos0:pos0 + T] = y[:, :, 2].reshape(B, T, H * d)
    return q, k, v


def rowstats_ref(stored):
    """{sum, sum of squares} per 64-column slot of the stored rows: [M, N/64, 2]"""
    M, N = stored.shape
    s = stored.view(M, N // 64, 64)
    return torch.stack([s.sum(-1), (s * s).sum(-1)], -1)


def stats_ref(stored, eps):
    """{mean, rstd} of the rows (population variance), float64 [M, 2]"""
    mean = stored.mean(1)
    var = (stored * stored).mean(1) - mean * mean
    return torch.stack([mean, 1.0 / torch.sqrt(var + eps)], 1)


def rowstats32_ref(a, w, bias, x32, a_map=None):
    """the fp32 stream x32 + a.w^T + bias (to be updated in place) and its 16-bit copy's source: the SAME values, rounded once by the
    caller with to16; partial sums from the fp32 values"""
    new = x32 + pre_act_ref(a, w, bias, a_map)
    return new, rowstats_ref(new)


def rms_ssq_ref(stored16, n_wg_cols=16):
    """producer partials ssq_out[b][m] = sum over workgroup b's output columns (16 each, the last one ragged) of the ROUNDED output
    squared: [ceil(N/16), M]"""
    M, N = stored16.shape
    nb = -(-N // n_wg_cols)
    pad = torch.zeros((M, nb * n_wg_cols), dtype=F64, device=stored16.device)
    pad[:, :N] = stored16 * stored16
    return pad.view(M, nb, n_wg_cols).sum(-1).T.contiguous()


def rms_rstd_ref(ssq_in, K, eps):
    """consumer: rstd_m = rsqrt(sum_b ssq_in[b][m] / K + eps), [M]"""
    return 1.0 / torch.sqrt(ssq_in.sum(0) / K + eps)


def rms_ref(a, w, ssq_in, eps, resid=None, swiglu=False):
    """haff_gemm_*_rms consumer in float64: epi(rstd_m * (a . w^T))"""
    M, K = a.shape
    y = a @ w.T
    if ssq_in is not None:
        y = rms_rstd_ref(ssq_in[:, :M], K, eps)[:, None] * y
    y = swiglu_ref(y) if swiglu else y
    return y if resid is None else y + resid


def batched_ref(A, W, C, lda, sAo, sAi, ldw, sWo, sWi, ldc, sCo, sCi, nb_outer, nb_inner, M, N, K):
    """C_z = A_z . W_z^T on FLAT float64 buffers with element strides (zero strides included); returns a copy of C"""
    out = C.clone()
    for zo in range(nb_outer):
        for zi in range(nb_inner):
            a = torch.as_strided(A, (M, K), (lda, 1), zo * sAo + zi * sAi)
            w = torch.as_strided(W, (N, K), (ldw, 1), zo * sWo + zi * sWi)
            torch.as_strided(out, (M, N), (ldc, 1), zo * sCo + zi * sCi).copy_(a @ w.T)
    return out


# ---------------------------------------------------------------------------------------------------------------- builders
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randint(shape, g, lo, hi):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def check_exact_bound(a, w, gran=1.0):
    """every partial sum of a @ w.T is a multiple of gran and bounded by |a| @ |w|.T: fp32 holds it exactly below 2^24 gran"""
    assert (a.abs() @ w.abs().T).max().item() < 2.0 ** 24 * gran


def ints(M, N, K, seed, lo=-4, hi=4):
    """dense integer operands in [lo, hi]: (a [M, K], w [N, K])"""
    g = _gen(seed)
    a, w = _randint((M, K), g, lo, hi), _randint((N, K), g, lo, hi)
    assert is16(a, BF16) and is16(w, BF16) and is16(a, F16) and is16(w, F16)
    check_exact_bound(a, w)
    return a, w


def small_ints(M, N, K, seed, limit=232.0):
    """integer operands shrunk so that max |a . w^T| <= limit (asserted): entries in [-r, r] with r in 2, 1 and `a` thinned out, so
    that the accumulator's deviation sqrt(K q var_a var_w) stays below limit / 7. The epilogue cases add an integer bias in [-8, 8]
    and an integer residual in [-16, 16] to it and stay at |y| <= 256, where bf16 (and fp16) holds every integer."""
    g = _gen(seed)
    q, r = 1.0, 2
    var = {2: 2.0, 1: 2.0 / 3.0}
    sd_max = limit / 7.0
    if K * var[r] * var[r] > sd_max ** 2:
        r = 1
    q = min(1.0, sd_max ** 2 / (K * var[r] * var[r]))
    a, w = _randint((M, K), g, -r, r), _randint((N, K), g, -r, r)
    if q < 1.0:
        a = a * (torch.rand((M, K), generator=g) < q).double()
    check_exact_bound(a, w)
    assert (a @ w.T).abs().max().item() <= limit
    return a, w


def round_bf16(M, N, K, seed):
    """entries in [-2, 2], a[:, 0] = 256 and w[:, 0] cycling +-{1.5, 1, 1.25, 1.75}: the exact results fill (256, 512), where bf16
    holds only even integers — odd ones are ties. Asserts the shares the case is there for."""
    g = _gen(seed)
    a, w = _randint((M, K), g, -2, 2), _randint((N, K), g, -2, 2)
    a[:, 0] = 256.0
    cyc = torch.tensor([1.5, -1.5, 1.0, -1.0, 1.25, -1.25, 1.75, -1.75], dtype=F64)
    w[:, 0] = cyc[torch.arange(N) % 8]
    assert is16(a, BF16) and is16(w, BF16)
    check_exact_bound(a, w, 0.25)
    exact = a @ w.T
    ties = ((exact.abs() > 256) & (exact.abs() < 512) & (exact % 2 == 1)).double().mean().item()
    want = to16(exact, BF16, exact=True)
    differs = (trunc_bf16(exact) != want).double().mean().item()
    assert ties >= 0.25 and differs >= 0.10, (ties, differs)
    return a, w


def once(M, N, K, seed, dtype=BF16):
    """ROUNDS ONCE: a small_ints product with every other weight doubled (an even base, |base| <= 120) and two reserved columns:
    a[:, 0] = 128, w[:, 0] = +-3 by column and a[:, 1] = w[:, 1] = 1, so that the accumulator +-384 + 1 + base is an ODD integer in
    (256, 512), a tie of bf16 (fp16: a[:, 0] = 1024, ties in (2048, 4096)). The residual is +-1: 257 + 1 = 258 is a bf16 value,
    rounding 257 first gives 256 and then 256 + 1 -> 256. Returns (a, w, resid) and asserts that the rounded-twice restatement
    differs from to16(exact) on >= 10 % of the elements."""
    g = _gen(seed)
    a, w = small_ints(M, N, K, seed + 1, limit=60.0)
    w = w * 2.0
    a[:, 0] = 128.0 if dtype == BF16 else 1024.0
    w[:, 0] = torch.where(torch.arange(N) % 2 == 0, 3.0, -3.0).double()
    a[:, 1], w[:, 1] = 1.0, 1.0
    assert is16(a, dtype) and is16(w, dtype)
    check_exact_bound(a, w)
    acc = a @ w.T
    lo = 256.0 if dtype == BF16 else 2048.0
    assert bool((acc % 2 == 1).all()) and acc.abs().min().item() > lo and acc.abs().max().item() < 2 * lo
    resid = torch.where(_randint((M, N), g, 0, 1) > 0, 1.0, -1.0).double()
    twice = to16(to16(acc, dtype).double() + resid, dtype)
    share = (twice != to16(acc + resid, dtype, exact=True)).double().mean().item()
    assert share >= 0.10, share
    return a, w, resid


def top_bf16(M, N, K, seed):
    """The top of the format: a[:, 0] = a[:, 1] = 2^120, w[:, 0] = +-2^7 * 255/128, w[:, 1] in {0, +-2^-1} by column, the rest small
    integers. Columns with w1 = 0 give +-2^127 * 255/128, the largest finite bf16, which must stay finite and exact; columns with
    w1 = +-2^-1 of the same sign give +-0x7F7F8000, a tie: finite in f32, +-inf in bf16. The small terms lie below half an fp32 ulp
    of the sum (2^103) and cannot move it in any order. Nothing is NaN. Returns (a, w, expected f32 as float64)."""
    g = _gen(seed)
    a, w = _randint((M, K), g, -4, 4), _randint((N, K), g, -4, 4)
    n = torch.arange(N)
    sign = torch.where(n % 2 == 0, 1.0, -1.0).double()
    a[:, 0] = a[:, 1] = 2.0 ** 120
    w[:, 0] = sign * 2.0 ** 7 * 255.0 / 128.0
    w[:, 1] = torch.where((n // 2) % 2 == 0, 0.0, 0.5).double() * sign
    assert is16(a, BF16) and is16(w, BF16)
    big = a[:, :2] @ w[:, :2].T
    small = (a[:, 2:].abs() @ w[:, 2:].abs().T).max().item()
    assert small < 2.0 ** 102                                       # far below half an ulp (2^103) of the fp32 sum
    assert is16(big, F32) and bool(torch.isfinite(big.float()).all())
    want16 = big.float().to(BF16)
    assert bool((want16.abs() == 2.0 ** 127 * 255.0 / 128.0).any()) and bool(torch.isinf(want16).any())
    assert not bool(torch.isnan(want16).any())
    return a, w, big


def coded_bias(N):
    return ((torch.arange(N) % 17) - 8).double()


def coded_resid(R, N):
    r, n = torch.arange(R)[:, None], torch.arange(N)[None, :]
    return (((3 * r + 5 * n) % 33) - 16).double()


def coded_stats(M, rms=False):
    m = torch.arange(M)
    mean = torch.zeros(M, dtype=F64) if rms else ((m % 7) - 3).double()
    rstd = torch.pow(2.0, ((m % 5) - 3).double())
    return torch.stack([mean, rstd], 1)


def coded_a_map(M, rows, seed):
    """gather map with repeats: M draws from `rows` source rows (rows < M forces repeats), int32"""
    return torch.randint(0, rows, (M,), generator=_gen(seed)).to(torch.int32)


def coded_row_map(M, seed, extra=37, drop=0.07):
    """a permutation into M + extra rows with about 7 % of the entries -1, int32; returns (row_map, rows of the output)"""
    g = _gen(seed)
    rm = torch.randperm(M + extra, generator=g)[:M]
    rm[torch.rand((M,), generator=g) < drop] = -1
    if M > 2:
        rm[M // 2] = -1                                             # at least one dropped row at every size
    return rm.to(torch.int32), M + extra


def ln_exact(M, N, K, seed, rms=False):
    """ints operands with mean integer in [-3, 3], rstd a power of two in [2^-3, 2], colsum = sum_k w exact, integer bias:
    rstd * (acc - mean * colsum) + bias is exact in fp32 whatever the FMA grouping (every intermediate is a multiple of 2^-3 below
    2^21). Returns dict(a, w, bias, ln_stats, ln_colsum)."""
    a, w = ints(M, N, K, seed)
    stats = coded_stats(M, rms)
    colsum = None if rms else w.sum(1)
    bias = coded_bias(N)
    pre = pre_act_ref(a, w, bias, None, stats, colsum)
    big = (a.abs() @ w.abs().T).max().item() + 3.0 * w.abs().sum(1).max().item()
    assert big < 2.0 ** 21 and is16(pre, F32)
    return dict(a=a, w=w, bias=bias, ln_stats=stats, ln_colsum=colsum)


def acts(M, N, K, seed, ln=False):
    """pre-activations that are integers in [-48, 48] scaled by 1/4, so that the curved part of each activation is sampled and the
    pre-activation itself is exact in fp32: small_ints (|acc| <= 40) with w / 4 and a coded bias / 4. ln: with coded statistics whose
    rstd is scaled by the power of two that brings 2 max|acc - mean colsum| below 10, and the exact column sums. Returns
    dict(a, w, bias[, ln_stats, ln_colsum]) and asserts |pre| <= 12, the range B_GELU was evaluated over."""
    a, w = small_ints(M, N, K, seed, limit=40.0)
    c = dict(a=a, w=w * 0.25, bias=coded_bias(N) * 0.25)
    if ln:
        c["w"], st = w, coded_stats(M)
        raw = (a @ w.T - st[:, 0:1] * w.sum(1)[None, :]).abs().max().item()
        st[:, 1] *= 2.0 ** -math.ceil(math.log2(2.0 * raw / 10.0))
        c.update(ln_stats=st, ln_colsum=w.sum(1))
    pre = pre_act_ref(c["a"], c["w"], c["bias"], None, c.get("ln_stats"), c.get("ln_colsum"))
    assert pre.abs().max().item() <= X_MAX and is16(pre, F32) and is16(c["w"], BF16) and is16(c["w"], F16)
    assert (pre.abs() < 4).double().mean().item() > 0.25          # the curved part
    return c


ROPE_PAIRS = torch.tensor([[1.0, 0.0], [0.0, 1.0], [0.0, -1.0], [-1.0, 0.0], [0.5, 0.5], [0.5, -0.5]], dtype=F64)


def rope_exact(Tmax):
    """[Tmax, cos(0..63) | sin(0..63)] with (cos, sin) of (position p, column c) = ROPE_PAIRS[(3 p + 5 c) mod 6]: another pair at
    p +- 1 and at c +- 1, every product with an integer exact"""
    p, c = torch.arange(Tmax)[:, None], torch.arange(64)[None, :]
    pair = ROPE_PAIRS[(3 * p + 5 * c) % 6]                          # [Tmax, 64, 2]
    return torch.cat([pair[..., 0], pair[..., 1]], 1).contiguous()


# ------------------------------------------------------------------------------------------------------------------ bounds
# erf(z) = z P(z^2) on |z| <= 3 (clamped), the degree-8 fit of gemm_act<GELU>: the coefficient VALUES, highest degree first
GELU_POLY = (4.9182759198629356e-08, -2.2677306787954876e-06, 4.6147291868692264e-05, -0.0005535572418011725,
             0.004437862429767847, -0.02564961276948452, 0.11186250299215317, -0.3758186101913452, 1.1283628940582275)
# absolute, for |x| <= X_MAX = 12: the polynomial with its clamp at |z| = 3 in float32 against exact erf stays below 9e-5 there, with
# a peak at |x| = 4.24 where the clamp sets in. Past the clamp the computed erf is a constant 1 - d (d = 1.4e-5 ... 1.5e-5 by the
# rounding of the evaluation), so the error is 0.5 |x| d: 8.8e-5 at |x| = 12, and above 1e-4 from |x| = 13.6 on (1.18e-4 measured
# at 16 on the MI355X). The cases therefore keep |x| <= 12; bound() refuses anything wider.
B_GELU = 1.0e-4
X_MAX = 12.0
B_EXP_REL = 2.0 ** -17   # relative to |x|: one-ulp v_exp_f32 and v_rcp_f32, the argument scaling and two roundings < 2^-19; x 4


def gelu_poly_f32(x32):
    """the polynomial GELU evaluated in float32 as the kernel writes it"""
    z = torch.clamp(x32 * torch.tensor(0.70710678118654752440, dtype=F32), -3.0, 3.0)
    u = z * z
    pz = torch.full_like(u, GELU_POLY[0])
    for c in GELU_POLY[1:]:
        pz = pz * u + torch.tensor(c, dtype=F32)
    hx = 0.5 * x32
    return hx + hx * (z * pz)


def bound(pre, act, up=None):
    """admissible |f32 value - float64 result| of the three transcendental activations at pre-activation `pre` (|pre| <= 12 for
    GELU, <= 16 for the exponential forms); SwiGLU: b_silu(gate) * |up|"""
    assert pre.abs().max().item() <= (X_MAX if act == ACT_GELU else 16.0)
    if act == ACT_GELU:
        return torch.full_like(pre, B_GELU)
    if act in (ACT_QUICK_GELU, ACT_SILU):
        b = B_EXP_REL * pre.abs()
        return b if up is None else b * up.abs()
    raise ValueError(act)


def interval16(ref, b, dtype):
    """16-bit output: one rounding of an admissible f32 value, [to16(ref - b), to16(ref + b)], no further ulp"""
    return to16(ref - b, dtype), to16(ref + b, dtype)


# ----------------------------------------------------------------------------------------------------------------- dispatch
def dispatch(M, N, K, tile_cfg=0, workspace=False, swiglu=False, ln=False, a_map=False):
    """The branch gemm_bf16_impl takes: a Python mirror of its rules, of launch_skinny (NT = 1 / 2 / 4) and of launch_skinny_splitk
    (nt, ks). Names: skinny_mt{1,2,4}_nt{1,2,4}, skinny_splitk_nt{4,2}_ks{4,2}, tile_splitk_{slices}x{K-tiles}[_short],
    tile128[_deep], tile256, tile192."""
    ws_bytes = WS_BYTES if workspace else 0
    tile_rows = M > 32 and workspace and K % BK == 0 and not ln and (N >= 8192 or K >= 8192)
    if M <= 64 and K % 128 == 0 and tile_cfg == 0 and not (M > 32 and N >= 16384) and not tile_rows:
        tiles = (N + 15) // 16
        if M > 32 and workspace and ws_bytes >= 16 * M * N and not a_map and not swiglu and not ln and N <= 8192:
            for nt in (4, 2):
                for ks in (4, 2):
                    if K % (128 * ks) == 0 and 192 <= (tiles + nt - 1) // nt * ks <= 640:
                        return f"skinny_splitk_nt{nt}_ks{ks}"
        mt = 1 if M <= 16 else 2 if M <= 32 else 4
        nt4, nt2 = mt >= 2 and tiles // 4 >= 192, mt >= 2 and tiles // 2 >= 192
        nt = (4 if nt4 else 2) if swiglu else (4 if nt4 else 2 if nt2 else 1)
        return f"skinny_mt{mt}_nt{nt}"
    if tile_cfg == 0 and workspace and not ln and M > 32 and K % BK == 0:
        t128, ksteps = -(-M // 128) * -(-N // 128), K // BK
        if t128 <= 256 and ksteps >= 32:
            for c in (16, 8, 4, 2):
                kc = -(-ksteps // c)
                n_sl = -(-ksteps // kc)
                last = ksteps - (n_sl - 1) * kc
                if kc >= 4 and last >= 2 and t128 * n_sl <= 512 and 4 * n_sl * M * N <= ws_bytes:
                    return f"tile_splitk_{n_sl}x{kc}" + ("_short" if last != kc else "")
    big_ok = K % BK == 0                                             # (operands below 4 GiB: every case here)
    big, mid = tile_cfg == 2 and big_ok, tile_cfg == 3 and big_ok
    if tile_cfg == 0 and big_ok:
        t128 = -(-M // 128) * -(-N // 128)
        t256 = -(-M // 256) * -(-N // 256)
        t192 = -(-M // 192) * -(-N // 256)
        e128 = t128 / (-(-t128 // 512) * 512)
        e256 = t256 / (-(-t256 // 256) * 256) * 1.22
        e192 = t192 / (-(-t192 // 256) * 256) * 1.22 * 0.93
        big = M >= 256 and N >= 256 and e256 > e128
        if M >= 192 and N >= 256 and not ln and e192 > 1.05 * max(e256, e128):
            mid, big = True, False
    if mid:
        return "tile192"
    if big:
        return "tile256"
    tiles = -(-M // 128) * -(-N // 128)
    return "tile128_deep" if tiles <= 1024 and -(-K // BK) >= 3 else "tile128"


def tiles_per_workgroup(M, N, branch, cap=256):
    """tiles the busiest workgroup of a persistent 8-wave launch takes under a stream cap"""
    bm = 192 if branch == "tile192" else 256
    return -(-(-(-M // bm) * -(-N // 256)) // cap)


def nt_store(M, n_out, out_f32):
    """launches whose output takes the non-temporal stores: 64 MiB and more"""
    return M * n_out * (4 if out_f32 else 2) >= (64 << 20)


SPEC256 = {  # the HAFF_SPEC instances by feature set: (bias, ln, csum, res, stat, res32, map, hm, rope, act, swiglu) -> needs whole M tiles
    "bias_ln_csum": True, "bias_ln_csum_map_hm": True, "bias_ln_csum_gelu": True, "bias_res_stat": True, "bias_res_stat_res32": True,
    "rope": False, "res": False, "swiglu": False, "plain": False, "bias": False, "bias_res": False, "bias_qgelu": False}
SPEC192 = ("plain", "res", "swiglu", "bias", "bias_res")


def spec_instance(branch, M, N, ldc, out_f32, bias=False, ln=False, csum=False, res=False, ldr=0, stat=False, res32=False,
                  row_map=False, hm=False, rope=False, act=0, swiglu=False):
    """A PREDICTION of the specialised instance launch_gemm picks (a key of SPEC256 / an entry of SPEC192), or None for the generic
    instance. The library does not report which instance ran, so this is a second restatement of the HAFF_SPEC / HAFF_SPEC192 lists
    and of launch_gemm's `ok` contract, compared with them by hand: an instance added there has to be added to SPEC256 / SPEC192
    here, or the lists the GPU file prints fall behind without a test failing. The rule:
    16-bit output, N % 256 == 0, ldc and ldr multiples of 8 (the callers here keep every base 16-byte aligned), and a feature set
    that has an instance; the instances without GF_RAGM need M % 256 == 0."""
    if branch not in ("tile256", "tile192") or out_f32 or N % 256 or ldc % 8 or (res and not res32 and ldr % 8) or (csum and not ln):
        return None
    parts = [n for n, on in (("bias", bias), ("ln", ln), ("csum", csum), ("res", res or res32), ("stat", stat), ("res32", res32),
                             ("map", row_map), ("hm", hm), ("rope", rope)) if on]
    parts += {0: [], ACT_GELU: ["gelu"], ACT_QUICK_GELU: ["qgelu"], ACT_RELU: ["relu"], ACT_SILU: ["silu"]}[act]
    parts += ["swiglu"] if swiglu else []
    key = "_".join(parts) or "plain"
    if branch == "tile192":
        return key if key in SPEC192 else None
    if key in SPEC256 and (M % 256 == 0 or not SPEC256[key]):
        return key
    return None


# ------------------------------------------------------------------------------------------------------------ branch table
# name -> (M, N, K, tile_cfg, what dispatch() must answer). ops.linear passes the workspace for 32 < M <= 1024 without a tile_cfg.
BRANCHES = {
    "skinny_mt1_m1": (1, 1024, 128, 0, "skinny_mt1_nt1"),
    "skinny_mt1": (16, 1000, 384, 0, "skinny_mt1_nt1"),
    "skinny_mt2_nt1": (17, 1024, 1024, 0, "skinny_mt2_nt1"),
    "skinny_mt2_nt2": (32, 6144, 128, 0, "skinny_mt2_nt2"),
    "skinny_mt2_nt4": (17, 12288, 128, 0, "skinny_mt2_nt4"),
    "skinny_mt4": (48, 1024, 1024, 0, "skinny_mt4_nt1"),
    "skinny_splitk_nt4_ks4": (48, 4096, 4096, 0, "skinny_splitk_nt4_ks4"),
    "skinny_splitk_nt2_ks4": (48, 2048, 512, 0, "skinny_splitk_nt2_ks4"),
    "skinny_splitk_ks2": (48, 6144, 256, 0, "skinny_splitk_nt4_ks2"),
    "tile_splitk": (288, 1024, 4096, 0, "tile_splitk_16x4"),
    "tile_splitk_short_last_slice": (288, 1024, 2368, 0, "tile_splitk_8x5_short"),   # 37 K-tiles: 7 slices of 5 and one of 2
    "tile128": (300, 520, 256, 1, "tile128_deep"),
    "tile128_ktail": (300, 520, 72, 1, "tile128"),
    "tile128_two_ktiles": (300, 520, 128, 1, "tile128"),
    "tile256": (512, 520, 256, 2, "tile256"),
    "tile256_spec": (512, 512, 256, 2, "tile256"),
    "tile256_ragm": (582, 512, 256, 2, "tile256"),
    "tile256_one_ktile": (512, 512, 64, 2, "tile256"),
    "tile192": (400, 512, 256, 3, "tile192"),
    "tile192_ragged_n": (401, 520, 128, 3, "tile192"),
}
# too large for a CPU reference per parameter: operands and float64 reference are built once on the device
BIG = {
    "tile128_many": (4224, 4224, 192, 1, "tile128"),      # 1089 tiles: the deep-K loop is off by count
    "nt_store_16": (8192, 4096, 64, 0, "tile256"),        # 64 MiB of 16-bit output: non-temporal stores
    "nt_store_f32": (4096, 4096, 64, 0, "tile256"),       # 64 MiB of fp32 output
}
PERSISTENT = {"persistent256": (1024, 1024, 128, 2, "tile256"), "persistent192": (1152, 1024, 128, 3, "tile192")}   # under gemm_stream_cap(8)
# entry points that take no tile_cfg (gather, folded norm) pick their tile by shape
AUTO = {
    "skinny": (5, 1000, 256, 0, "skinny_mt1_nt1"),
    "auto128": (300, 520, 256, 0, "tile128_deep"),
    "auto256": (300, 264, 256, 0, "tile256"),                # ragged M and N: the generic 8-wave instance
    "auto192": (400, 264, 256, 0, "tile192"),                # gather only (a folded norm never takes the 192-row tile)
    "auto256_spec": (2816, 3072, 64, 0, "tile256"),          # 132 whole tiles: the least at which the auto rule takes the 8-wave tile
    "auto256_spec_ring": (2816, 3072, 256, 0, "tile256"),    # the same tiles (the rule does not look at K) over four K-tiles: the ring loop
}


def uses_workspace(M, tile_cfg, ln=False, a_map=False):
    return 32 < M <= 1024 and not tile_cfg and not ln and not a_map


def reaches(name, table=None, **kw):
    """(M, N, K, tile_cfg) of a table entry, once the mirror is seen to agree with the branch the entry is listed for"""
    M, N, K, cfg, want = (table or BRANCHES)[name]
    got = dispatch(M, N, K, cfg, workspace=uses_workspace(M, cfg, kw.get("ln", False), kw.get("a_map", False)), **kw)
    assert got == want, (name, got, want)
    return M, N, K, cfg
