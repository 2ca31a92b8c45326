"""Plain CPU restatements of the backward, loss and optimiser kernels of csrc/train.hip, with the inputs that put those kernels
at their edges and the bounds the comparisons use.

Every function is written from the operation's formula (the comments of train.hip, the reference's LISA.py / llava_llama.py,
torch.optim.AdamW) with torch on the CPU. Each takes `dt`: torch.float64 is the reference, torch.float32 is the same formula with
every operation rounded to fp32, in the kernel's order where the order matters — the error of that evaluation against float64 is
what the bounds are built from (`bound`). Keyword flags switch on one deliberate mistake each; tests/test_train_edge_ref_cpu.py
shows that every one of them misses the bound. Nothing here imports the package or touches a GPU.
"""
import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24          # unit roundoff of fp32
K = 4                     # the bound is K times the fp32 evaluation's own worst error ...
FLOOR_ULPS = 8            # ... plus this many fp32 ulps (2 * U32 each) of the scale, for the device's expf / erff / logf
NAN, INF = float("nan"), float("inf")
F32, F64, BF16, F16 = torch.float32, torch.float64, torch.bfloat16, torch.float16
DTYPES = (F32, BF16, F16)
CODE = {BF16: 0, F32: 1, F16: 3}
IDS = {F32: "f32", BF16: "bf16", F16: "f16"}
ACT_NONE, ACT_GELU, ACT_QUICK_GELU, ACT_RELU, ACT_SILU = 0, 1, 2, 3, 4
ACTS = (ACT_NONE, ACT_GELU, ACT_QUICK_GELU, ACT_RELU, ACT_SILU, 7)     # 7: an unknown code is the identity
SENT = 7.0                # what the over-allocated output buffers are filled with
GRID_CAP = 16384 * 256    # threads of one sweep of the grid-stride kernels


def rand(shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


def f32(v):
    """the fp32 value a c_float argument carries, as a Python float"""
    return float(np.float32(v))


# ---------------------------------------------------------------------------------------------------------------- bounds
def half_ulp(ref, dtype):
    """half the spacing of `dtype` at |ref| (float64 tensor): the rounding of a stored result. 0 for fp32, whose own rounding is
    part of the fp32 evaluation's error."""
    if dtype == F32:
        return torch.zeros_like(ref)
    p, emin = (8, -126) if dtype == BF16 else (11, -14)
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** emin))).clamp_min(emin)
    return torch.pow(2.0, e - p)


def bound(ref, ev32, dtype=F32, scale=None, rowwise=False):
    """Elementwise bound on |kernel - ref|: K * max|ev32 - ref| + FLOOR_ULPS fp32 ulps of the scale + half an ulp of the storage
    type at the reference value. The maxima and the scale (default max|ref|) are taken over the tensor, or over each row."""
    ref = ref.double()
    fin = torch.isfinite(ref)
    err = torch.where(fin, (ev32.double() - ref).abs(), torch.zeros_like(ref))
    mag = torch.where(fin, ref.abs(), torch.zeros_like(ref))
    if rowwise:
        err, mag = err.amax(-1, keepdim=True), mag.amax(-1, keepdim=True)
    else:
        err, mag = err.max(), mag.max()
    if scale is not None:
        mag = torch.as_tensor(scale, dtype=F64)
    return K * err + FLOOR_ULPS * 2 * U32 * mag + half_ulp(ref, dtype) + 1e-300


def ratio(got, ref, bnd):
    """max |got - ref| / bnd over the finite entries of ref; inf if got is not finite there, or differs from ref where ref is
    inf / NaN."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    fin = torch.isfinite(ref)
    if not bool(torch.isfinite(got[fin]).all()):
        return INF
    if not torch.equal(torch.nan_to_num(got[~fin], nan=1.5e300), torch.nan_to_num(ref[~fin], nan=1.5e300)):
        return INF
    if not bool(fin.any()):
        return 0.0
    bnd = torch.as_tensor(bnd, dtype=F64).expand_as(ref)
    return ((got - ref).abs()[fin] / bnd[fin]).max().item()


def sum_bound_abs(ev32, ref, abs_sum, chain=0):
    """Bound for a sum of fp32 terms whose float64 sum of absolute values is abs_sum: K times the error of an fp32 sum of the same
    terms (ev32: seq_sum32, one term after the other — not any kernel's order, only a sample of what fp32 addition loses on these
    terms) plus FLOOR_ULPS ulps of abs_sum. chain: for the forms that finish with `chain` fp32 atomic adds on ONE address, in
    whatever order the waves arrive, chain * U32 * abs_sum is added: each add rounds the running sum once, by at most U32 of
    abs_sum, and with near-equal addends the roundings do not cancel (65539 equal terms: 10 times the bound without this term).
    That is the worst case, and at chain in the thousands it is wide (4096 * U32 = 2.4e-4): there the tests add inputs whose sums
    are exact in any order and compare those with ==. The ordered forms, and atomic forms with a few adds per address, take 0."""
    return K * (ev32.double() - ref).abs() + (FLOOR_ULPS * 2 + chain) * U32 * abs_sum + 1e-300


def sum_bound(terms, ev32, ref, dim=0, chain=0):
    """sum_bound_abs for the sum of `terms` along dim"""
    return sum_bound_abs(ev32, ref, terms.double().abs().sum(dim), chain)


def seq_sum32(terms, dim=0):
    """the fp32 sum of `terms` along dim, added one after the other"""
    return terms.float().cumsum(dim).select(dim, -1)


def wave_sum(v):
    """sum over the last axis the way one 64-lane wave does it: lane l adds elements l, l + 64, ... in turn, then the xor tree"""
    C = v.shape[-1]
    n = -(-C // 64)
    p = F.pad(v, (0, n * 64 - C)).reshape(*v.shape[:-1], n, 64)
    acc = torch.zeros_like(p[..., 0, :])
    for i in range(n):
        acc = acc + p[..., i, :]
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., idx ^ o]
    return acc[..., 0]


# ----------------------------------------------------------------------------------------------------------- elementwise
EDGE_X = (0.0, -0.0, 1e-3, -1e-3, 1.0, -1.0, 20.0, -20.0, 100.0, -100.0)
ELEMENTWISE_N = (1, 255, 257)
ELEMENTWISE_BIG = GRID_CAP + 257


def edge_values(n, seed, dtype):
    """[n] in `dtype`: the edge values in turn (starting at `seed`), N(0, 2) on every third position once all of them fit"""
    v = torch.tensor(EDGE_X)[(torch.arange(n) + seed) % len(EDGE_X)]
    if n > len(EDGE_X):
        r = rand((n,), seed, 2.0)
        v = torch.where(torch.arange(n) % 3 == 1, r, v)
    return v.to(dtype)


def sigmoid(x):
    return 1.0 / (1.0 + torch.exp(-x))


def act_fwd(x, act, dt=F64):
    x = x.to(dt)
    if act == ACT_GELU:
        return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440))
    if act == ACT_QUICK_GELU:
        return x / (1.0 + torch.exp(-1.702 * x))
    if act == ACT_RELU:
        return torch.clamp_min(x, 0.0)
    if act == ACT_SILU:
        return x / (1.0 + torch.exp(-x))
    return x.clone()


def act_grad(x, act, dt=F64):
    x = x.to(dt)
    if act == ACT_GELU:
        cdf = 0.5 * (1.0 + torch.erf(x * 0.70710678118654752440))
        pdf = 0.39894228040143267794 * torch.exp(-0.5 * x * x)
        return cdf + x * pdf
    if act == ACT_RELU:
        return (x > 0).to(dt)
    if act == ACT_SILU:
        s = sigmoid(x)
        return s * (1.0 + x * (1.0 - s))
    if act == ACT_QUICK_GELU:
        s = sigmoid(1.702 * x)
        return s * (1.0 + 1.702 * x * (1.0 - s))
    return torch.ones_like(x)


def act_bwd(x, dy, act, dt=F64):
    return dy.to(dt) * act_grad(x, act, dt)


def axpby(a, b, alpha, beta, dt=F64):
    out = f32(alpha) * a.to(dt)
    return out if b is None else out + f32(beta) * b.to(dt)


def scale_rows(a, alpha, stride, dt=F64):
    """a [rows, cols] * alpha[r * stride] (alpha fp32)"""
    al = alpha.to(dt)
    return a.to(dt) * (al[0] if stride == 0 else al[:a.shape[0], None])


# ---------------------------------------------------------------------------------------------------------------- SwiGLU
SWIGLU_F = (16, 48, 11008)
SWIGLU_M = (1, 3)


def swiglu_inputs(M, Fd, seed, dtype):
    """gu [M, 2F] (16-column groups gate | up) and dy [M, F]; the first gates are +-100, +-20, +-0"""
    gu, dy = rand((M, 2 * Fd), seed, 2.0), rand((M, Fd), seed + 1)
    gu[:, :6] = torch.tensor([100.0, -100.0, 20.0, -20.0, 0.0, -0.0])
    return gu.to(dtype), dy.to(dtype)


def _split_gu(gu, swapped=False):
    M = gu.shape[0]
    v = gu.reshape(M, -1, 2, 16)
    g, u = v[:, :, 0].reshape(M, -1), v[:, :, 1].reshape(M, -1)
    return (u, g) if swapped else (g, u)


def swiglu_fwd(gu, dt=F64, swapped=False):
    g, u = _split_gu(gu.to(dt), swapped)
    return g / (1.0 + torch.exp(-g)) * u


def swiglu_bwd(gu, dy, dt=F64, swapped=False):
    """closed form; -> dgu [M, 2F] in gu's layout"""
    g, u = _split_gu(gu.to(dt), swapped)
    d = dy.to(dt)
    s = sigmoid(g)
    dg, du = d * u * s * (1.0 + g * (1.0 - s)), d * g * s
    if swapped:
        dg, du = du, dg
    M = gu.shape[0]
    return torch.stack([dg.reshape(M, -1, 16), du.reshape(M, -1, 16)], 2).reshape(M, -1)


def autograd_of(fn, x, upstream):
    """d <fn(x), upstream> / dx in float64"""
    x = x.double().clone().requires_grad_(True)
    fn(x).backward(upstream.double())
    return x.grad


# ------------------------------------------------------------------------------------------------------------- transpose
TRANSPOSE_CASES = ((1, 1, 1, 1, 1), (1, 33, 4, 40, 33), (31, 32, 31, 32, 37), (32, 31, 40, 31, 31), (33, 1, 33, 8, 3),
                   (33, 33, 64, 40, 35), (32, 32, 32, 32, 32))     # (R, C, Rp, Cp, ld_in)


def transpose(x, Rp, Cp):
    """x [..., R, C] -> [..., Cp, Rp], zero padded; a copy"""
    R, C = x.shape[-2:]
    return F.pad(x.transpose(-1, -2), (0, Rp - R, 0, Cp - C))


# ----------------------------------------------------------------------------------------------------------------- norms
NORM_GENERIC = ((1, 1), (5, 63), (4, 64), (7, 65), (3, 4097))
NORM_VEC = ((1, 4096), (5, 5120))
EPS_LN, EPS_RMS = 1e-5, 1e-6


def norm_inputs(rows, C, seed, dtype):
    """x, dy [rows, C] in dtype, w fp32 [C] with a zero and a negative entry, add [rows, C]. Row 0 of x is constant (variance 0,
    rstd = eps^-1/2; the constant 3 keeps every partial sum exact); in fp32 the last row has mean 100 and spread 1e-2."""
    x, dy, w = rand((rows, C), seed), rand((rows, C), seed + 1), 1.0 + 0.3 * rand((C,), seed + 2)
    w[0] = 0.0
    w[C // 2] = -0.75 if C > 1 else w[C // 2]
    x[0] = 3.0
    if dtype == F32 and rows > 1:
        x[-1] = 100.0 + 1e-2 * x[-1]
    return x.to(dtype), dy.to(dtype), w, rand((rows, C), seed + 3).to(dtype)


def norm_fwd(x, w, rms, eps):
    if rms:
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * w
    return F.layer_norm(x, x.shape[-1:], w, None, eps)


def norm_bwd(x, dy, w, rms, eps, add=None, dt=F64, ln_without_mean_g=False, rms_with_mean_g=False):
    """closed form (train.hip): xhat = (x - mean) * rstd, g = dy * w;
    LayerNorm dx = rstd * (g - mean(g) - xhat * mean(g * xhat)); RMSNorm (mean = 0) dx = rstd * (g - xhat * mean(g * xhat)).
    -> dx (+ add), dyx = dy * xhat. Row sums in the generic kernel's order."""
    x, dy, w = x.to(dt), dy.to(dt), w.to(dt)
    C = x.shape[-1]
    if rms:
        mean = torch.zeros_like(x[:, :1])
        rstd = 1.0 / torch.sqrt(wave_sum(x * x)[:, None] / C + eps)
    else:
        mean = wave_sum(x)[:, None] / C
        rstd = 1.0 / torch.sqrt(wave_sum((x - mean) ** 2)[:, None] / C + eps)
    xh = (x - mean) * rstd
    g = dy * w
    a, b = wave_sum(g)[:, None] / C, wave_sum(g * xh)[:, None] / C
    use_a = (not rms and not ln_without_mean_g) or (rms and rms_with_mean_g)
    dx = rstd * (g - (a if use_a else 0.0) - xh * b)
    if add is not None:
        dx = dx + add.to(dt)
    return dx, dy * xh


# --------------------------------------------------------------------------------------------------------------- softmax
SOFTMAX_NQ, SOFTMAX_ROWS = 5, 2 * 3 * 5 + 1
SOFTMAX_NK = (1, 63, 64, 65, 130)
SOFTMAX_SCALE = 0.125


def softmax_modes(Nk):
    """(causal, q_pos0)"""
    return ((0, 0), (1, 0), (1, 3), (1, Nk - SOFTMAX_NQ))


def softmax_lim(rows, Nq, Nk, causal, q_pos0, lim_off=0, div=False):
    r = torch.arange(rows)
    q = (r // Nq) if div else (r % Nq)
    return torch.clamp(q + q_pos0 + 1 + lim_off, max=Nk) if causal else torch.full((rows,), Nk)


def softmax_scores(rows, Nk, ld, lim, seed):
    """fp32 [rows, ld]: N(0, 4) * 8 in the visible columns, row 1 with one score 60 / scale above the rest, NaN in the masked-out
    and the padding columns"""
    s = rand((rows, ld), seed, 32.0)
    if rows > 1:
        s[1, 0] += 60.0 / SOFTMAX_SCALE
    j = torch.arange(ld)[None, :]
    return torch.where(j < lim[:, None], s, torch.full_like(s, NAN))


def softmax_fwd(s, Nk, ldp, lim, scale, dt=F64):
    """[rows, ldp]: softmax(scale * s) over each row's first lim columns, zeros beyond (a row with no visible key is all zeros)"""
    rows = s.shape[0]
    j = torch.arange(Nk)[None, :]
    vis = j < lim[:, None]
    z = torch.where(vis, s[:, :Nk].to(dt) * f32(scale), torch.full((rows, Nk), -INF, dtype=dt))
    m = z.amax(-1, keepdim=True)
    m = torch.where(torch.isfinite(m), m, torch.zeros_like(m))
    e = torch.where(vis, torch.exp(z - m), torch.zeros_like(z))
    tot = wave_sum(e)[:, None]
    p = torch.where(vis, e * (1.0 / torch.where(tot > 0, tot, torch.ones_like(tot))), torch.zeros_like(e))
    return F.pad(p, (0, ldp - Nk))


def softmax_bwd(p, dp, Nk, ldp, scale, dt=F64):
    """dS = scale * P o (dP - rowsum(dP o P)) over the first Nk columns, zeros up to ldp"""
    pv, d = p[:, :Nk].to(dt), dp[:, :Nk].to(dt)
    dot = wave_sum(pv * d)[:, None]
    return F.pad(f32(scale) * pv * (d - dot), (0, ldp - Nk))


# ------------------------------------------------------------------------------------------------------------------ RoPE
ROPE_D = (2, 8, 128)
ROPE_H, ROPE_T, ROPE_ROWS = 3, 5, 15
ROPE_POS0 = (0, 7)


def rope_table(Tmax, d):
    """fp32 [Tmax, d] = cos(d/2) | sin(d/2), base 10000 (an input of the kernel: the reference reads the same fp32 values)"""
    inv = 1.0 / (10000.0 ** (torch.arange(0, d, 2).double() / d))
    ang = torch.arange(Tmax).double()[:, None] * inv[None, :]
    return torch.cat([ang.cos(), ang.sin()], 1).float().contiguous()


def rope(x, cs, Tlen, H, d, pos0, adjoint, dt=F64, drop_pos0=False, keep_sign=False):
    """rotate-half RoPE of x [rows, H*d] at position pos0 + row % Tlen; the adjoint rotates back (sin -> -sin)"""
    rows = x.shape[0]
    v = x.to(dt).reshape(rows, H, d)
    pos = (0 if drop_pos0 else pos0) + torch.arange(rows) % Tlen
    half = d // 2
    co, si = cs.to(dt)[pos][:, None, :half], cs.to(dt)[pos][:, None, half:]
    if adjoint and not keep_sign:
        si = -si
    x1, x2 = v[..., :half], v[..., half:]
    return torch.cat([x1 * co - x2 * si, x2 * co + x1 * si], -1).reshape(rows, H * d)


# --------------------------------------------------------------------------------------------------------- cross-entropy
CE_V = (1, 255, 256, 257, 32003)
CE_GSCALE = 0.37


def ce_inputs(V, seed, dtype):
    """logits [6, V] in dtype and labels: label 0, label V - 1, ignored, a row of equal logits, a row whose label's logit is 30
    above the rest, and the same row with another label"""
    x = rand((6, V), seed, 2.0)
    x[3] = -1.25
    x[4, V // 3] += 30.0
    x[5] = x[4]
    labels = torch.tensor([0, V - 1, -100, V // 2, V // 3, (V // 3 + 1) % V])
    return x.to(dtype), labels


def ce_extreme(dtype):
    """two rows of V = 257 at the type's edge: f16 at +-65504, fp32 / bf16 near -1e4; the second row is ignored"""
    V = 257
    if dtype == F16:
        x = torch.full((2, V), 65504.0)
        x[:, 1::2] = -65504.0
    else:
        x = -1e4 + rand((2, V), 3, 2.0)
    return x.to(dtype), torch.tensor([V - 1, -100])


def cross_entropy(x, labels, gscale, dt=F64, onehot_shift=0):
    """row loss = logsumexp(x) - x[label], d = (softmax(x) - onehot(label)) * gscale; both exactly zero where label < 0.
    The sums in the kernel's order: thread t of 256 takes columns t, t + 256, ..., four wave trees, then the four waves."""
    x = x.to(dt)
    R, V = x.shape
    m = x.amax(-1, keepdim=True)
    n = -(-V // 256)
    e = F.pad(torch.exp(x - m), (0, n * 256 - V)).reshape(R, n, 4, 64)
    acc = torch.zeros((R, 4, 64), dtype=dt)
    for i in range(n):
        acc = acc + e[:, i]
    idx = torch.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        acc = acc + acc[..., idx ^ o]
    tot = acc[:, 0, 0] + acc[:, 1, 0] + acc[:, 2, 0] + acc[:, 3, 0]
    lse = m[:, 0] + torch.log(tot)
    valid = labels >= 0
    lab = labels.clamp_min(0)
    loss = torch.where(valid, lse - x[torch.arange(R), lab], torch.zeros_like(lse))
    onehot = F.one_hot((lab + onehot_shift) % V, V).to(dt)
    d = (torch.exp(x - lse[:, None]) - onehot) * f32(gscale)
    return loss, torch.where(valid[:, None], d, torch.zeros_like(d))


# ----------------------------------------------------------------------------------------------------------- mask losses
MASK_N = (1, 255, 256 * 256 + 3)
MASK_WGT = (1.0, 0.0, 2.0)


def mask_inputs(n, seed):
    """x, t fp32 [3, n]: logits N(0, 3) with +-100 among them; targets all 0, all 1, mixed"""
    x = rand((3, n), seed, 3.0)
    x[:, 1::7] = 100.0
    x[:, 3::11] = -100.0
    t = torch.zeros((3, n))
    t[1] = 1.0
    t[2] = (rand((n,), seed + 1) > 0).float()
    return x, t


def mask_terms(x, t, wgt, dt=F64):
    """[3, n, 4]: the summands of [bce_sum, sum(p t), sum(p), sum(t)] with z = wgt * x, p = sigmoid(z)"""
    z, t = f32(wgt) * x.to(dt), t.to(dt)
    p = sigmoid(z)
    bce = torch.clamp_min(z, 0.0) - z * t + torch.log1p(torch.exp(-z.abs()))
    return torch.stack([bce, p * t, p, t], -1)


def mask_losses(stats, n, wrong_n=None, no_1000=False):
    """[bce, dice] per sample from stats [S, 4] (LISA.py): bce = bce_sum / n, dice = 1 - (2 sum(p t)/1000 + eps) / (sum(p)/1000 +
    sum(t)/1000 + eps)"""
    k = 1.0 if no_1000 else 1000.0
    bce = stats[:, 0] / (wrong_n or n)
    dice = 1.0 - (2.0 * stats[:, 1] / k + 1e-6) / (stats[:, 2] / k + stats[:, 3] / k + 1e-6)
    return bce, dice


def mask_grad(x, t, stats, wgt, c_bce, c_dice, dt=F64, wrong_n=None, no_1000=False):
    """closed form of d (sum_s c_bce[s] bce_s + c_dice[s] dice_s) / dx from the given statistics; c_* are [S] tensors"""
    x, t, stats = x.to(dt), t.to(dt), stats.to(dt)
    n = x.shape[1]
    k = 1.0 if no_1000 else 1000.0
    z = f32(wgt) * x
    p = sigmoid(z)
    num = (2.0 * stats[:, 1] / k + 1e-6)[:, None]
    den = (stats[:, 2] / k + stats[:, 3] / k + 1e-6)[:, None]
    ddice_dp = -(2.0 * t / k) / den + num / (den * den) / k
    return f32(wgt) * (c_bce.to(dt)[:, None] * (p - t) / float(wrong_n or n) + c_dice.to(dt)[:, None] * ddice_dp * p * (1.0 - p))


def mask_grad_autograd(x, t, wgt, c_bce, c_dice):
    def fn(xx):
        bce, dice = mask_losses(mask_terms(xx, t, wgt).sum(1), xx.shape[1])
        return (c_bce.double() * bce + c_dice.double() * dice).sum()
    return autograd_of(fn, x, torch.tensor(1.0))


# -------------------------------------------------------------------------------------------------------------- taxonomy
TAX_C, TAX_ROWS = (1, 4, 8), (1, 64, 65)


def taxonomy_inputs(rows, C, seed, soft):
    z = rand((rows, C), seed, 2.0)
    if soft:
        t = torch.rand((rows, C), generator=torch.Generator().manual_seed(seed + 1)) * 0.7      # sums to anything but 1
    else:
        t = F.one_hot(torch.arange(rows) % C, C).float()
    return z, t


def taxonomy_ce(z, t, dt=F64):
    """CrossEntropyLoss applied to the already soft-maxed probabilities (LISA.py): p = softmax(z),
    loss = -sum_c t_c log_softmax(p)_c -> (p, loss, dloss/dz in closed form)"""
    z, t = z.to(dt), t.to(dt)
    e = torch.exp(z - z.amax(-1, keepdim=True))
    p = e / e.sum(-1, keepdim=True)
    q = torch.exp(p - p.amax(-1, keepdim=True))
    s2 = q.sum(-1, keepdim=True)
    lse2 = p.amax(-1, keepdim=True) + torch.log(s2)
    loss = -(t * (p - lse2)).sum(-1)
    gp = -t + t.sum(-1, keepdim=True) * q / s2
    return p, loss, p * (gp - (gp * p).sum(-1, keepdim=True))


def taxonomy_loss(z, t):
    return -(t.double() * torch.log_softmax(torch.softmax(z.double(), -1), -1)).sum(-1)


# ------------------------------------------------------------------------------------------------------ bilinear adjoint
RESIZE_BWD_BIG = (1, (2049, 2050), (2049, 2048), (40, 48))     # 4.196 M crop pixels: past the 16384 x 256 threads of one sweep


def resize_bwd(g, src_hw, crop_hw, dt=F64, half_pixel=True, clamp_to_crop=True):
    """adjoint of bilinear(align_corners=False) from the crop of a [N, Hs, Ws] source to g [N, Ho, Wo], as a scatter of the
    forward's taps: f = max(s (o + 0.5) - 0.5, 0), i0 = min(int(f), crop - 1), i1 = min(i0 + 1, crop - 1), l = f - i0.
    -> [N, Hs, Ws], zero outside the crop. The two flags are the two mistakes the bound has to catch."""
    N, Ho, Wo = g.shape

    def axis(crop, out, src):
        s = torch.tensor(float(crop), dtype=dt) / torch.tensor(float(out), dtype=dt)
        f = torch.clamp_min(s * (torch.arange(out, dtype=dt) + (0.5 if half_pixel else 0.0)) - 0.5, 0.0)
        i0 = torch.clamp(f.long(), max=crop - 1)
        i1 = torch.clamp(i0 + 1, max=(crop if clamp_to_crop else src) - 1)
        l1 = f - i0.to(dt)
        return i0, i1, 1.0 - l1, l1
    y0, y1, hy, ly = axis(crop_hw[0], Ho, src_hw[0])
    x0, x1, hx, lx = axis(crop_hw[1], Wo, src_hw[1])
    g = g.to(dt)
    din = torch.zeros((N, src_hw[0] * src_hw[1]), dtype=dt)
    for yi, wy in ((y0, hy), (y1, ly)):
        for xi, wx in ((x0, hx), (x1, lx)):
            idx = (yi[:, None] * src_hw[1] + xi[None, :]).reshape(-1)
            din.index_add_(1, idx, (g * wy[None, :, None] * wx[None, None, :]).reshape(N, -1))
    return din.view(N, *src_hw)


def resize_bwd_autograd(g, src_hw, crop_hw):
    def fn(x):
        return F.interpolate(x[:, None, :crop_hw[0], :crop_hw[1]], tuple(g.shape[1:]), mode="bilinear", align_corners=False)[:, 0]
    return autograd_of(fn, torch.zeros((g.shape[0], *src_hw)), g)


# ------------------------------------------------------------------------------------------------------------- scatter
SCATTER_C = (1, 255, 256, 257)
SCATTER_V = 9


def scatter_ids():
    V = SCATTER_V
    return {"ignored": torch.tensor([3, -200, 5, -100, 3, 0, -100, 8]), "one id": torch.full((70,), 4), "first and last": torch.tensor([0, V - 1, V - 1, 0, 0]),
            "one row": torch.tensor([V - 1])}


def scatter_add(ids, dx, dE0):
    """float64 dE0 + sum of the rows of dx whose id is >= 0, at that id"""
    keep = ids >= 0
    return dE0.double().clone().index_add_(0, ids[keep], dx.double()[keep])


def scatter_abs(ids, dx, dE0):
    keep = ids >= 0
    return dE0.double().abs().index_add_(0, ids[keep], dx.double().abs()[keep])


# ----------------------------------------------------------------------------------------------------------- reductions
COLSUM_GENERIC = ((1, 1), (255, 63), (257, 65))
COLSUM_VEC = ((1024, 8), (1031, 128), (4099, 256), (1025, 2048))
COLSUM_PARTS_R = (1, 64, 65, 4096, 4097, 65536, 70001)
REDUCE_PARTS = (1, 63, 64, 65, 300)
SUMSQ_N = (1, 255, 256, 257, 1024 * 256 + 5)


# ----------------------------------------------------------------------------------------------------------------- AdamW
ADAMW_N = (1, 257)
ADAMW_BIG = GRID_CAP + 257
ADAMW_LR, ADAMW_EPS = 0.05, 1e-8


def adamw_inputs(n, seed, g_dtype):
    """master N(0, 1), first moment N(0, 0.1), second moment >= 0, gradient in g_dtype; element 0 (and every 97th) has a zero
    gradient on zero moments"""
    w, m, v, g = rand((n,), seed), rand((n,), seed + 1, 0.1), rand((n,), seed + 2, 0.1).pow(2), rand((n,), seed + 3)
    for t in (m, v, g):
        t[::97] = 0.0
    return w, m, v, g.to(g_dtype)


def adamw(w, m, v, g, lr, b1, b2, eps, wd, step, gscale, dt=F64, bc_step_off=0, decay_after=False):
    """torch.optim.AdamW, one step: w *= 1 - lr wd; m = b1 m + (1 - b1) g; v = b2 v + (1 - b2) g^2;
    w -= lr (m / (1 - b1^t)) / (sqrt(v / (1 - b2^t)) + eps). The scalars arrive as fp32; g is scaled by gscale first."""
    lr, b1, b2, eps, wd = (f32(s) for s in (lr, b1, b2, eps, wd))
    w, m, v = w.to(dt), m.to(dt), v.to(dt)
    gr = g.to(dt) * gscale
    t = step + bc_step_off
    if dt == F32:
        bc1, bc2 = float(np.float32(1) - np.power(np.float32(b1), np.float32(t))), float(np.float32(1) - np.power(np.float32(b2), np.float32(t)))
    else:
        bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    if not decay_after:
        w = w - lr * wd * w
    m = b1 * m + (1.0 - b1) * gr
    v = b2 * v + (1.0 - b2) * gr * gr
    w = w - lr * (m / bc1) / (torch.sqrt(v / bc2) + eps)
    if decay_after:
        w = w - lr * wd * w
    return w, m, v


# ---------------------------------------------------------------------------------------------------------- expectations
def expect(fn, *args, dtypes=(F32,), rowwise=False, scales=None, **kw):
    """[(float64 reference, elementwise bound)] for each output of fn: the reference is fn in float64, the bound comes from fn in
    fp32 (`bound`). dtypes: the storage type of each output; scales: an explicit scale for the floor of each (default max|ref|)."""
    ref, ev = fn(*args, dt=F64, **kw), fn(*args, dt=F32, **kw)
    if not isinstance(ref, tuple):
        ref, ev = (ref,), (ev,)
    scales = scales or (None,) * len(ref)
    return [(r, bound(r, e, d, s, rowwise)) for r, e, d, s in zip(ref, ev, dtypes, scales)]


def ce_scales(x, gscale):
    """per row: the loss is a difference of numbers of the logits' size, and the gradient's exponent carries that difference"""
    big = x.double().abs().amax(-1).clamp_min(1.0)
    return big, (big * f32(gscale))[:, None]
