"""Plain CPU restatements of the TN weight-gradient product (csrc/gemm_tn.hip) and of the flash attention pair (the lse forward of
csrc/attention.hip and csrc/attention_bwd.hip), with the inputs that put those kernels at their edges, the shape lists and the
bounds the comparisons use. Built on tests/train_edge_ref.py (bound, sum_bound_abs, ratio, half_ulp, K = 4, FLOOR_ULPS = 8).

gemm_tn(a, b, dt): a^T b; float64 is the reference, the fp32 evaluation adds the rows one after the other.

attn(...): out, lse2, dq, dk, dv of softmax(scale q k^T [causal]) v from the closed form, [B][H][N][128] operands. float64 is the
reference. With r16 = BF16 | F16 the same formula is evaluated in fp32 with the roundings the kernels document and no others (listed
at `attn`); the error of that evaluation against float64 plays the part the fp32 evaluation plays in train_edge_ref: per output row
    bound = K * max_row |rounded evaluation - float64| + FLOOR_ULPS fp32 ulps of the row's scale + half a storage ulp.
The row's scale is the sum of the absolute values of the terms the row's largest entry is a sum of (`attn_scales`): dq, dk and dv
are sums that cancel (a query that sees one key has dP = delta, so dS = 0 in exact arithmetic and a few fp32 ulps of |dP| + |delta|
in any fp32 evaluation), and what fp32 addition loses is proportional to the terms, not to the sum. lse2 is stored in fp32, so it
has no storage term; a row of it is the [Nq] row of one (batch, head), a single number having no maximum to take.
Keyword flags switch on one deliberate mistake each (MISTAKES); tests/test_flash_tn_ref_cpu.py shows that every one of them misses
the bound on the trap inputs, and that a second correct evaluation in the kernels' own block order stays inside it.
Nothing here imports the package or touches a GPU."""
import numpy as np
import torch

from train_edge_ref import BF16, F16, F32, F64, INF, NAN, bound, f32, half_ulp, rand, sum_bound_abs  # noqa: F401

LOG2E = 1.4426950408889634
LN2 = 0.6931471805599453
D = 128                   # head dim of the flash pair
HALF = (BF16, F16)
IDS = {BF16: "bf16", F16: "f16"}


# ---------------------------------------------------------------------------------------------------------------- gemm_tn
TT, TR = 128, 64          # output tile edge, contraction rows per slab (gemm_tn.hip)


def tn_geometry(M, N1, N2):
    """(rows_per_split, splits) as tn_geometry of gemm_tn.hip states them: 512 workgroups wanted, at most 64 splits, a split a
    multiple of 64 rows and at least 256"""
    tiles = -(-N1 // TT) * -(-N2 // TT)
    want = max(1, min(64, -(-512 // tiles)))
    rps = max(4 * TR, -(-(-(-M // want)) // TR) * TR)
    return rps, -(-M // rps)


# M, the contraction length. At N1 = N2 = 8 (one tile: 64 splits wanted):
TN_M = (1,        # one slab of one row: 63 zero rows fetched past m_hi (`in = m < m_hi`)
        63, 64,   # the slab's last row absent / present
        65,       # a second slab of one row: `if (m0 + TR < m_hi) fetch(m0 + TR)`
        255,      # rows_per_split = 256 (the floor `rps < 4 * TR`): one split, its fourth slab one row short
        256,      # one split, exactly full
        257,      # a second split that owns one row: blockIdx.z = 1, m_lo = 256, m_hi clipped to M
        16385,    # want = 64 (the cap): rows_per_split = roundup(ceil(16385 / 64) = 257, 64) = 320 -> 52 splits, the last of 65 rows
        20000)    # rows_per_split = roundup(313, 64) = 320 -> 63 splits, the last of 160 rows = 2 slabs + 32 rows; 320 does not divide M
TN_M_SHORT = (1, 65, 257)     # the M the wider outputs and the layouts are run at
TN_N = ((8, 8),               # one tile, 120 of its 128 columns absent on both sides (`a_ok`, `b_ok`, `if (i >= p.N1) continue`)
        (128, 128),           # one whole tile
        (136, 264),           # 2 x 3 tiles, the last of each side cut at 8 columns
        (8, 2048))            # 1 x 16 tiles: 32 splits wanted
TN_BIG = (64, 2048, 2056)     # N1 * N2 = 4 210 688 > 4096 * 256 * 4: gemm_tn_reduce_kernel's grid-stride loop takes a second trip
assert tn_geometry(255, 8, 8) == (256, 1) and tn_geometry(257, 8, 8) == (256, 2)
assert tn_geometry(16385, 8, 8) == (320, 52) and tn_geometry(20000, 8, 8) == (320, 63) and 20000 % 320 == 160
assert TN_BIG[1] * TN_BIG[2] > 4096 * 256 * 4


def tn_exact_inputs(M, N1, N2, seed, dtype):
    """integers in [-4, 4]: every product (<= 16) and every partial sum (<= 16 M <= 2^24 for M <= 2^20) is exact in fp32, in any
    order, so the fp32 result equals the float64 product"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randint(-4, 5, (M, N1), generator=g).to(dtype), torch.randint(-4, 5, (M, N2), generator=g).to(dtype))


def tn_gauss_inputs(M, N1, N2, seed, dtype):
    return rand((M, N1), seed).to(dtype), rand((M, N2), seed + 1).to(dtype)


def gemm_tn(a, b, dt=F64, drop_row=None, double_row=None):
    """a [M, N1], b [M, N2] -> a^T b in dt. fp32: the rows added one after the other. The two flags are the two mistakes a slab or
    split edge can make: row m left out, row m counted twice."""
    a, b = a.to(dt), b.to(dt)
    if dt == F64:
        out = a.T @ b
    else:
        out = torch.zeros((a.shape[1], b.shape[1]), dtype=dt)
        for m in range(a.shape[0]):
            out += a[m][:, None] * b[m][None, :]
    if drop_row is not None:
        out = out - a[drop_row][:, None] * b[drop_row][None, :]
    if double_row is not None:
        out = out + a[double_row][:, None] * b[double_row][None, :]
    return out


def tn_expect(a, b, dtype):
    """(float64 reference, elementwise bound) for Gaussian operands and a result stored in dtype: sum_bound with chain = 0 (the
    split partials are added in index order) plus half a storage ulp"""
    ref = gemm_tn(a, b)
    return ref, sum_bound_abs(gemm_tn(a, b, F32), ref, a.double().abs().T @ b.double().abs()) + half_ulp(ref, dtype)


def tn_edge_rows(M, N1, N2):
    """the first and last row of the first slab, of the first split, and of the last (ragged) slab and split"""
    rps, splits = tn_geometry(M, N1, N2)
    rows = {0, TR - 1, TR, rps - 1, rps, (splits - 1) * rps, (M - 1) // TR * TR, M - 1}
    return sorted(r for r in rows if 0 <= r < M)


# ------------------------------------------------------------------------------------------------------------- flash pair
MISTAKES = ("mask_lt",             # key j visible iff j < i + q_pos0 (for <=)
            "mask_plus1",          # ... iff j <= i + q_pos0 + 1
            "no_q_pos0",           # q_pos0 taken as 0
            "drop_key63",          # the last key of every 64-block invisible
            "drop_query63",        # the last query row of every 64-block missing from dk / dv
            "natural_lse",         # lse in the natural log (returned, and used by the backward as the trainer would feed it)
            "no_ds_scale",         # dS = P (dP - delta), the scale missing
            "delta_other_head",    # delta from the next head's out
            "dq_first_block")      # dq without the contribution of key blocks j > 0

# (B, H, Nq, Nk, causal, q_pos0, ld - H * 128). Forward: 128-query workgroups, 64-key tiles; backward: 64 x 64 blocks.
FLASH_SHAPES = (
    (1, 1, 1, 1, 1, 0, 0),         # one query, one key: every other row and key of the tiles is padding (`qrow < Nq`, `key < Nk`)
    (1, 1, 1, 129, 1, 128, 0),     # one query that sees 129 keys: forward nkt = 3 from `last_key / KT + 1`, the third tile one key
    (1, 1, 63, 64, 1, 1, 0),       # q_pos0 = Nk - Nq = 1: the last query sees key 63, the last of the only block
    (1, 2, 64, 64, 1, 0, 64),      # whole blocks, ld = H * 128 + 64
    (1, 1, 65, 65, 1, 0, 0),       # key block 1 holds one key, seen by one query: backward i0 = 64 / 64 = 1
    (1, 1, 65, 63, 0, 0, 0),       # non-causal Nq > Nk, the key tile one short (`kt * KT + KT > Nk`)
    (1, 3, 127, 128, 0, 0, 0),     # non-causal Nq < Nk, query block one short
    (1, 1, 128, 127, 0, 0, 64),    # the forward's query block exactly full
    (1, 3, 129, 129, 1, 0, 64),    # a second 128-query workgroup of one row, B * H = 3: grid decoded as id / nqb
    (2, 4, 130, 130, 1, 0, 0),     # B * H = 8 with nqb = 2: the grid decoded as (id & 7) + 8 * (id / (8 * nqb))
    (1, 1, 130, 70, 0, 0, 0),      # non-causal Nq > Nk across a query-block edge
    (1, 1, 70, 133, 1, 63, 0),     # q_pos0 = Nk - Nq: every key is seen, the causal diagonal crosses both key-block edges
    (1, 2, 70, 133, 1, 10, 64),    # 0 < q_pos0 < Nk - Nq: keys 80 .. 132 are seen by no query (dk = dv = 0), forward nkt = 2 of 3
    (1, 1, 70, 200, 1, 0, 0),      # q_pos0 = 0, Nk > Nq: backward key blocks 2 and 3 start at i0 = 2, 3 >= nqb = 2: empty loop
    (2, 8, 131, 131, 1, 0, 0),     # B * H = 16, Nq > 128
    (1, 1, 330, 333, 1, 3, 0),     # 6 key blocks, 3 query workgroups, ragged both ways
)
FLASH_SCALE = D ** -0.5
TRAP_C = 0.3


def flash_id(s):
    return "B%dH%d-%dx%d-%s%d-ld+%d" % (s[0], s[1], s[2], s[3], "causal" if s[4] else "full", s[5], s[6])


def visible(Nq, Nk, causal, q_pos0, mask_lt=False, mask_plus1=False, no_q_pos0=False, drop_key63=False):
    """bool [Nq, Nk]: key j visible to query i iff j <= i + q_pos0 (causal), every key otherwise"""
    i, j = torch.arange(Nq)[:, None], torch.arange(Nk)[None, :]
    vis = torch.ones((Nq, Nk), dtype=torch.bool)
    if causal:
        lim = i + (0 if no_q_pos0 else q_pos0) + (1 if mask_plus1 else 0)
        vis = (j < lim) if mask_lt else (j <= lim)
    if drop_key63:
        vis = vis & (j % 64 != 63)
    return vis


def smooth_inputs(B, H, Nq, Nk, seed, r16):
    """q, do [B, H, Nq, 128], k, v [B, H, Nk, 128]: plain Gaussians, already values of r16"""
    return (rand((B, H, Nq, D), seed).to(r16), rand((B, H, Nk, D), seed + 1).to(r16), rand((B, H, Nk, D), seed + 2).to(r16),
            rand((B, H, Nq, D), seed + 3).to(r16))


def trap_inputs(B, H, Nq, Nk, q_pos0, seed, r16, c=TRAP_C):
    """Gaussian 16-bit values with c * (k[i + q_pos0] + k[min(i + q_pos0 + 1, Nk - 1)]) added to query i: the last key a causal
    query sees carries a large share of its row, and the first masked key would carry as much if it were seen (with Gaussian
    operands alone every key carries about 1 / Nk, and a mask that is off by one key moves nothing)."""
    q, k, v, do = smooth_inputs(B, H, Nq, Nk, seed, r16)
    i = torch.arange(Nq)
    a, b = torch.clamp(i + q_pos0, 0, Nk - 1), torch.clamp(i + q_pos0 + 1, 0, Nk - 1)
    q = (q.float() + c * (k[:, :, a].float() + k[:, :, b].float())).to(r16)
    return q, k, v, do


ONEHOT_GAIN = 24.0
ONEHOT_MARGIN = 160.0     # log2 units; 2^-150 is already zero in fp32, so every other key's probability is exactly 0


def onehot_inputs(B, H, Nq, Nk, causal, q_pos0, seed, r16):
    """q = ONEHOT_GAIN * k[choice]: the chosen key scores ONEHOT_MARGIN log2 units above every other visible key (checked here in
    float64 on the rounded Qs), so P is exactly one-hot in fp32. Choices: keys 0, 63, 64, 127, 128, Nk - 1 and the causal
    diagonal in turn, the diagonal (causal) or Nk - 1 where the turn's key is not visible, and for the last query. dO: integers in [-3, 3], so every sum
    of rows of dO is exact. -> q, k, v, do, choice [Nq]"""
    _, k, v, _ = smooth_inputs(B, H, Nq, Nk, seed, r16)
    i = torch.arange(Nq)
    diag = torch.clamp(i + q_pos0, 0, Nk - 1) if causal else torch.full((Nq,), Nk - 1)
    cand = torch.tensor([0, 63, 64, 127, 128, Nk - 1, -1])[i % 7]
    choice = torch.where((cand < 0) | (cand > diag) | (cand >= Nk), diag, cand)
    choice[-1] = diag[-1]     # the last key any query sees is chosen by the last query
    q = (ONEHOT_GAIN * k[:, :, choice].float()).to(r16)
    g = torch.Generator(device="cpu").manual_seed(seed + 9)
    do = torch.randint(-3, 4, (B, H, Nq, D), generator=g).to(r16)
    qs = (q.float() * f32(np.float32(FLASH_SCALE) * np.float32(LOG2E))).to(r16).double()
    s = qs @ k.double().transpose(-1, -2)
    s = torch.where(visible(Nq, Nk, causal, q_pos0), s, torch.full_like(s, -INF))
    top = s.gather(-1, choice.expand(B, H, Nq)[..., None])
    rest = s.scatter(-1, choice.expand(B, H, Nq)[..., None], -INF).amax(-1, keepdim=True)
    assert float((top - rest).min()) >= ONEHOT_MARGIN, float((top - rest).min())
    return q, k, v, do, choice


def _sl2(scale, exact):
    """scale * log2(e): exactly (of the fp32 scale the entry point receives), or as the kernels form it, one fp32 product"""
    return f32(scale) * LOG2E if exact else float(np.float32(scale) * np.float32(LOG2E))


def attn(q, k, v, do, scale, causal, q_pos0, dt=F64, r16=None, **wrong):
    """-> out [B,H,Nq,128], lse2 [B,H,Nq], dq, dk, dv. lse2 = log2 sum_j 2^(scale log2e q.k_j) over the visible keys.
    r16 None: the closed form in dt (float64: the reference). r16 = BF16 | F16: fp32 arithmetic with the kernels' documented roundings:
      Qs = r16(fp32(q) * fp32(scale * log2e));  S = Qs k^T accumulated in fp32;
      forward: l sums the unrounded 2^(S - m), r16(2^(S - m)) multiplies V, out = r16(. / l);  delta = sum_c dO out from that out;
      backward: P = 2^(S - lse2), dS = P (dP - delta) scale in fp32; r16(P) multiplies dO, r16(dS) multiplies Q and K;
      dq, dk, dv = r16(fp32 sums)."""
    flags = dict.fromkeys(MISTAKES, False)
    assert set(wrong) <= set(MISTAKES), wrong
    flags.update(wrong)
    if r16 is not None:
        dt = F32
    rnd = (lambda x: x.to(r16).to(dt)) if r16 is not None else (lambda x: x)
    qf, kf, vf, dof = (t.to(dt) for t in (q, k, v, do))
    Nq, Nk = q.shape[2], k.shape[2]
    vis = visible(Nq, Nk, causal, q_pos0, flags["mask_lt"], flags["mask_plus1"], flags["no_q_pos0"], flags["drop_key63"])
    S = rnd(qf * _sl2(scale, r16 is None)) @ kf.transpose(-1, -2)
    S = torch.where(vis, S, torch.full_like(S, -INF))
    m = S.amax(-1, keepdim=True)
    e = torch.exp2(S - m)
    l = e.sum(-1, keepdim=True)
    lse2 = (m + torch.log2(l))[..., 0]
    out = rnd((rnd(e) @ vf) / l)
    if flags["natural_lse"]:
        lse2 = lse2 * LN2
    delta = (dof * (out.roll(-1, 1) if flags["delta_other_head"] else out)).sum(-1, keepdim=True)
    P = torch.exp2(S - lse2[..., None])
    dS = P * (dof @ vf.transpose(-1, -2) - delta) * (1.0 if flags["no_ds_scale"] else f32(scale))
    P, dS = rnd(P), rnd(dS)
    nb = 64 if flags["dq_first_block"] else Nk
    dq = dS[..., :nb] @ kf[..., :nb, :]
    if flags["drop_query63"]:
        keep = (torch.arange(Nq) % 64 != 63).to(dt)[:, None]
        P, dS = P * keep, dS * keep
    return out, lse2, rnd(dq), rnd(dS.transpose(-1, -2) @ qf), rnd(P.transpose(-1, -2) @ dof)


def attn_blocked(q, k, v, do, scale, causal, q_pos0, r16):
    """The same five results, correct, in the kernels' own order and fp32 accumulators: the forward walks 64-key tiles with a
    running maximum that moves only when a tile raises it (accumulators rescaled then); the backward recomputes P per 64 x 64 block
    from the forward's lse2 and adds the blocks' dq / dk / dv contributions one after the other. Not a reference: the second
    evaluation that shows the bound can be met."""
    rnd = lambda x: x.to(r16).float()   # noqa: E731
    qf, kf, vf, dof = (t.float() for t in (q, k, v, do))
    B, H, Nq, Nk = q.shape[0], q.shape[1], q.shape[2], k.shape[2]
    vis = visible(Nq, Nk, causal, q_pos0)
    qs = rnd(qf * _sl2(scale, False))
    m = torch.zeros((B, H, Nq, 1))
    l = torch.zeros((B, H, Nq, 1))
    acc = torch.zeros((B, H, Nq, D))
    for j0 in range(0, Nk, 64):
        s = qs @ kf[..., j0:j0 + 64, :].transpose(-1, -2)
        s = torch.where(vis[:, j0:j0 + 64], s, torch.full_like(s, -INF))
        mx = s.amax(-1, keepdim=True)
        m_new = torch.clamp_min(mx, -1e30) if j0 == 0 else torch.maximum(m, mx)
        alpha = torch.ones_like(m) if j0 == 0 else torch.exp2(m - m_new)
        e = torch.exp2(s - m_new)
        l = l * alpha + e.sum(-1, keepdim=True)
        acc = acc * alpha + rnd(e) @ vf[..., j0:j0 + 64, :]
        m = m_new
    out = rnd(acc * (1.0 / l))
    lse2 = (m + torch.log2(l))[..., 0]
    delta = (dof * out).sum(-1, keepdim=True)
    dq, dk, dv = torch.zeros((B, H, Nq, D)), torch.zeros((B, H, Nk, D)), torch.zeros((B, H, Nk, D))
    for j0 in range(0, Nk, 64):
        kj, vj = kf[..., j0:j0 + 64, :], vf[..., j0:j0 + 64, :]
        for i0 in range(0, Nq, 64):
            sl = slice(i0, i0 + 64)
            s = qs[..., sl, :] @ kj.transpose(-1, -2)
            p = torch.where(vis[sl, j0:j0 + 64], torch.exp2(s - lse2[..., sl, None]), torch.zeros_like(s))
            ds = p * (dof[..., sl, :] @ vj.transpose(-1, -2) - delta[..., sl, :]) * f32(scale)
            p, ds = rnd(p), rnd(ds)
            dv[..., j0:j0 + 64, :] += p.transpose(-1, -2) @ dof[..., sl, :]
            dk[..., j0:j0 + 64, :] += ds.transpose(-1, -2) @ qf[..., sl, :]
            dq[..., sl, :] += ds @ kj
    return out, lse2, rnd(dq), rnd(dk), rnd(dv)


def attn_scales(q, k, v, do, scale, causal, q_pos0):
    """The floor's scale of each row of out, lse2, dq, dk, dv (float64): the largest sum of absolute values of the terms an entry of
    the row is a sum of. out: sum_j P |v|; lse2: the largest |score| of the row (lse2 = m + log2 l, at least 1); with
    T = P (|dO| |v|^T + sum_c |dO out|) scale, the terms of dS: dq: T |k|, dk: T^T |q|, dv: P^T |dO|."""
    qd, kd, vd, dod = (t.double() for t in (q, k, v, do))
    vis = visible(q.shape[2], k.shape[2], causal, q_pos0)
    S = (qd * _sl2(scale, True)) @ kd.transpose(-1, -2)
    S = torch.where(vis, S, torch.full_like(S, -INF))
    P = torch.softmax(S * LN2, -1)
    out = P @ vd
    T = P * (dod.abs() @ vd.abs().transpose(-1, -2) + (dod * out).abs().sum(-1, keepdim=True)) * f32(scale)
    big = lambda x: x.amax(-1, keepdim=True)   # noqa: E731
    s_abs = torch.where(vis, S.abs(), torch.zeros_like(S)).amax(-1).clamp_min(1.0)
    return (big(P @ vd.abs()), s_abs, big(T @ kd.abs()), big(T.transpose(-1, -2) @ qd.abs()), big(P.transpose(-1, -2) @ dod.abs()))


RESULTS = ("out", "lse2", "dq", "dk", "dv")


def delta_terms(q, k, v, do, scale, causal, q_pos0, r16):
    """What the rounding of delta adds to the bounds of dq and dk (float64, elementwise). delta[i] = sum_c dO[i][c] out[i][c] is taken
    from the STORED out, which is off by half a storage ulp and by the 16-bit rounding of the probabilities that multiplied V:
        |d out[i][c]| <= half_ulp(out[i][c]) + sum_j half_ulp(P[i][j]) |v[j][c]|,      |d delta[i]| <= sum_c |dO[i][c]| |d out[i][c]|.
    That ONE number per query moves the whole row dq[i] = scale sum_j P[i][j] (dP[i][j] - delta[i]) k[j] by d delta[i] scale |sum_j
    P[i][j] k[j]|, and dk[j] by scale sum_i P[i][j] d delta[i] |q[i]|. K times the rounded evaluation's error does not cover it row
    by row: within a row the error is one draw, not the largest of 128, and the draw of the evaluation can be several times smaller
    than another correct evaluation's (attn_blocked, whose probabilities are rounded against the running maximum, stood at 1.07 of
    the bound without this term on dq row 73 of the 130 x 70 shape: the evaluation's own error in that row was 1.7e-5, its 1.1e-4)."""
    qd, kd, vd, dod = (t.double() for t in (q, k, v, do))
    vis = visible(q.shape[2], k.shape[2], causal, q_pos0)
    S = (qd * _sl2(scale, True)) @ kd.transpose(-1, -2)
    P = torch.softmax(torch.where(vis, S, torch.full_like(S, -INF)) * LN2, -1)
    out = P @ vd
    d_out = half_ulp(out, r16) + torch.where(vis, half_ulp(P, r16), torch.zeros_like(P)) @ vd.abs()
    d_delta = (dod.abs() * d_out).sum(-1, keepdim=True)
    return d_delta * f32(scale) * (P @ kd).abs(), f32(scale) * (P * d_delta).transpose(-1, -2) @ qd.abs()


def attn_expect(q, k, v, do, scale, causal, q_pos0, r16):
    """[(float64 reference, per-row bound)] for out, lse2, dq, dk, dv as the kernels store them (r16; lse2 fp32)"""
    ref = attn(q, k, v, do, scale, causal, q_pos0)
    ev = attn(q, k, v, do, scale, causal, q_pos0, r16=r16)
    sc = attn_scales(q, k, v, do, scale, causal, q_pos0)
    extra = dict(zip(("dq", "dk"), delta_terms(q, k, v, do, scale, causal, q_pos0, r16)))
    return [(r, bound(r, e, F32 if n == "lse2" else r16, s, rowwise=True) + extra.get(n, 0.0)) for n, r, e, s in zip(RESULTS, ref, ev, sc)]


def unseen_keys(Nq, Nk, causal, q_pos0):
    """bool [Nk]: keys no query sees"""
    return ~visible(Nq, Nk, causal, q_pos0).any(0)


def bwd_workspace_elems(B, H, Nq):
    """the header's formula: delta [B*H*Nq] rounded up to 4 values, then B*H*128*roundup(Nq, 64) fp32 dq sums"""
    return (B * H * Nq + 3) // 4 * 4 + B * H * 128 * (-(-Nq // 64) * 64)


def to_token_major(x, ld, fill=NAN):
    """[B, H, N, 128] -> [B, N, ld] with head h at columns h * 128 and `fill` in the columns past H * 128"""
    B, H, N, _ = x.shape
    t = torch.full((B, N, ld), fill, dtype=x.dtype)
    t[:, :, :H * D] = x.permute(0, 2, 1, 3).reshape(B, N, H * D)
    return t


def from_token_major(t, H):
    B, N, _ = t.shape
    return t[:, :, :H * D].reshape(B, N, H, D).permute(0, 2, 1, 3)
