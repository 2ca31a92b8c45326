"""Plain CPU restatement of the inference attention family (the generic flash kernel with its three rel-pos forms, the ViT-H global
ping-pong kernel and the three decode layouts of csrc/attention.hip, the window kernel of csrc/window_attention.hip, the two fp32
kernels of csrc/attention_f32.hip), with inputs whose right answer is ONE row of V, or the mean of TWO, the case lists and the bound.
With Gaussian operands every one of N keys carries about 1 / N of a row and a dropped, doubled or misplaced key moves the output by
|v| / N; here it moves it by about |v|.

attn_ref(q, k, v, scale, causal=, q_pos0=, relh=, relw=, S=, nk_rows=): float64 softmax(scale q k^T + relh[q, j // S] + relw[q, j % S]) v
over the visible keys (j <= i + q_pos0 when causal, j < nk_rows[b] when ragged), [B, H, N, d] operands, relh / relw [B, H, Nq, S].
Keyword flags switch on one deliberate mistake each (MISTAKES; `rel_row_plus1` lives in relpos_from_tables, `pad_as_zero` in
window_fill). attn_blocked is a second CORRECT evaluation: fp32, the kernels' documented roundings, 64 keys at a time with a running
maximum. tests/test_attn_edge_ref_cpu.py shows that the blocked evaluation stays inside the bound on every case and that every flag
misses it by 10x or more.

Inputs (all values already rounded to the operand type; every builder returns the chosen key per query and asserts its margin in
float64 on the Q as the 16-bit kernels round it, r16(q * fp32(scale * log2e)), AND on the unrounded q the decode / fp32 kernels use):
  select_by_qk        q_i = GAIN * k[choice_i]. K rows have one common norm (amp * sqrt(d), rounded), so the chosen key leads by
                      GAIN * |k|^2 (1 - cos) scale log2e: with plain Gaussian rows the lead at d <= 64 is 24 sqrt(d) log2e (1 - z /
                      sqrt(d)) and misses 160 for one pair in thousands; equal norms at amp 2 (d >= 64) and 4 (d < 64) keep it.
  select_by_bias      relh[i, kh*] = relw[i, kw*] = 120 nat (173 log2 units over the row and column mates), small Gaussian q, k
  select_by_tables_14 window kernel: one-hot tables and queries, k = 0: bias 144 ([kh == kh*] + [kw == kw*]), margin 207 log2 units
  select_by_tables_64 fused global kernel: sign-code tables 3 s_r, largest off-diagonal dot product 20 of 40: margin 259 log2 units
  pair_inputs         k[b] = k[a] bit for bit, q = GAIN * k[a]: out = (v[a] + v[b]) / 2; late_jump: key 0 scores 40 log2 units
                      below the pair, which then sits past the first 64-key tile, so the running maximum has to move
  ragged_poison       rows >= nk_rows[b] hold K = 2 k[choice], V = 1000 (they would win if seen), or NaN.
NaN rows past nk_rows[b] are IN contract on both ragged paths: attn_decode_kernel clamps every load to key Nk - 1 (Nk - 2 with fused
RoPE, whose newest row comes from registers), and attn_fwd_kernel's load_tile takes a tile as `plain` only when kt * 64 + 64 <= Nk with
Nk = min(nk_rows[b], p.Nk), and clamps every other row index to Nk - 1; nkt = ceil(Nk / 64) never reaches a tile past it. Production
caches are uninitialised there. The fp32 kernels loop j < Nk and never form such an address.

Bound, per element, from the formats alone: |got - ref| <= u * max |v rows involved| + one output ulp of |ref|. u covers one rounding
of P and one of the output: 2^-8 (bf16), 2^-11 (f16) for the kernels whose P.V product takes 16-bit probabilities, 2^-22 for the
decode and fp32 kernels, whose P stays fp32. EXACT (torch.equal with v[choice]) for one-hot inputs on
  the generic kernel   the chosen score is the tile maximum, so `sacc -= shift` leaves exactly 0, p = 2^0 = 1 packs exactly, every
                       other p = 2^(<= -160) = 0, earlier accumulators are multiplied by alpha = 2^(-delta) = 0, l = 1, 1 / l = 1;
  the decode kernels   p = 2^(s - m_new) = 1 for the running maximum itself, alpha and the merge weights 2^(m - m_all) are 0 or 1;
  the fp32 kernels     expf(0) = 1, expf(<= -110) = 0, sum = 1, inv = 1, fmaf(1, v, 0) = v and every other partial is 0.
The ping-pong kernel's lazy reference (PP_LAZY) makes p a power of two times a rounding and the window kernel is held to the same
bound. Nothing here imports the package or touches a GPU."""
import math

import numpy as np
import torch

from train_edge_ref import BF16, F16, F32, F64, INF, NAN, f32, rand  # noqa: F401
from flash_tn_ref import LOG2E, LN2, ONEHOT_GAIN, ONEHOT_MARGIN  # noqa: F401

GAIN, MARGIN = ONEHOT_GAIN, ONEHOT_MARGIN
HALF = (BF16, F16)
IDS = {BF16: "bf16", F16: "f16", F32: "f32"}
U16 = {BF16: 2.0 ** -8, F16: 2.0 ** -11}      # one rounding of P plus one of the output, 16-bit P.V kernels
U32 = 2.0 ** -22                              # P kept in fp32 (decode, fp32 kernels)
BIAS_ON = 120.0                               # nat
JUMP = 40.0                                   # log2 units the late_jump key scores below the pair
# 40 is also the ping-pong kernel's bf16 threshold for moving its lazy softmax reference (PP_LAZY; 15 in f16), a coincidence and not
# a design: once k[0] is rounded to bf16 the gaps run from about 39.3 to 40.6, so in bf16 about half of the (b, h) pairs of a JUMP
# case stay on the p = 2^40 path and half call move_reference. JUMP_CLEAR lies clear of both thresholds: every pair moves it.
JUMP_CLEAR = 60.0
JUMP_TOL = 4.0                                # what the 16-bit rounding of k[0] may move the gap by

MISTAKES = ("swap_hw",          # relh[j % S] + relw[j // S]
            "rel_row_plus1",    # rel-pos table row index off by one (relpos_from_tables)
            "key_plus1",        # v[j + 1] for v[j]
            "drop_last_key",    # the last visible key of the batch entry invisible
            "drop_key63",       # the last key of every 64-tile invisible
            "mask_lt",          # causal: j < i + q_pos0
            "no_q_pos0",        # q_pos0 taken as 0
            "nk_plus1",         # one more key than nk_rows[b]
            "nk_of_batch0",     # nk_rows[0] for every batch entry
            "next_head_v",      # V of the next head (of the next batch entry where H == 1)
            "pad_as_zero",      # padded window tokens read as zeros (window_fill)
            "drop_last_wave",   # the decode merge loses the last 16-key trip's partial
            "no_rescale")       # the accumulator is not rescaled when the running maximum moves


def sl2(scale):
    """scale * log2(e) as the kernels form it: one fp32 product"""
    return float(np.float32(scale) * np.float32(LOG2E))


def ulp(x, dtype):
    """the spacing of `dtype` at |x| (float64 tensor)"""
    mant, emin = {BF16: (7, -126), F16: (10, -14), F32: (23, -126)}[dtype]
    x = x.double().abs()
    e = torch.where(x == 0, torch.full_like(x, emin), torch.frexp(x)[1].double() - 1.0)
    return torch.exp2(torch.clamp_min(e, emin) - mant)


def bound(ref, vmax, dtype, u):
    return u * vmax.double() + ulp(ref, dtype)


def unit_rows(shape, seed, dtype, amp):
    """Gaussian directions at one common norm amp * sqrt(d), rounded to dtype"""
    g = rand(shape, seed).double()
    return (g / g.norm(dim=-1, keepdim=True) * math.sqrt(shape[-1]) * amp).to(dtype)


def amp_of(d):
    return 2.0 if d >= 64 else 4.0


class Case:
    """One problem: q [B,H,Nq,d], k, v [B,H,Nk,d] in `dtype`; relh / relw fp32 [B,H,Nq,S] or None; nk_rows list or None;
    choice [B,H,Nq]; mates bool [B,H,Nq,Nk] or None (keys that tie with the chosen one by construction); vmax [B,H,Nq,d]: the
    largest |v| among the rows the answer is made of; onehot: the answer is v[choice] exactly."""
    causal, q_pos0, relh, relw, S, nk_rows, mates, onehot, tab_h, tab_w, grid, is_pad, jump = False, 0, None, None, 0, None, None, True, None, None, 0, None, None

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def kwargs(self):
        return dict(causal=self.causal, q_pos0=self.q_pos0, relh=self.relh, relw=self.relw, S=self.S, nk_rows=self.nk_rows)

    def ref(self, **wrong):
        return attn_ref(self.q, self.k, self.v, self.scale, **self.kwargs(), **wrong)

    def v_choice(self):
        B, H, Nq, d = self.q.shape
        return self.v.gather(2, self.choice[..., None].expand(B, H, Nq, d))


# ------------------------------------------------------------------------------------------------------------- reference
def _visible(Nq, Nk, nk, causal, q_pos0, fl):
    i, j = torch.arange(Nq)[:, None], torch.arange(Nk)[None, :]
    vis = (j < nk).expand(Nq, Nk).clone()
    if causal:
        lim = i + (0 if fl["no_q_pos0"] else q_pos0)
        vis &= (j < lim) if fl["mask_lt"] else (j <= lim)
    if fl["drop_key63"]:
        vis &= (j % 64 != 63)
    if fl["drop_last_key"]:
        vis &= (j != nk - 1)
    if fl["drop_last_wave"]:
        vis &= (j < (nk - 1) // 16 * 16)
    return vis


def _online(s, v, dt, rnd_p, rescale=True):
    """s [Nq, Nk] scores in the log2 domain (-inf where masked), 64 keys at a time with a running maximum that moves only when a
    tile raises it; rnd_p rounds the probabilities that multiply V (l sums the unrounded ones). rescale=False is the `no_rescale`
    mistake: the maximum moves, the accumulators stay."""
    Nq, Nk = s.shape
    m = torch.full((Nq, 1), -1e30, dtype=dt)
    l = torch.zeros((Nq, 1), dtype=dt)
    acc = torch.zeros((Nq, v.shape[-1]), dtype=dt)
    for j0 in range(0, Nk, 64):
        t = s[:, j0:j0 + 64]
        m_new = torch.maximum(m, t.amax(-1, keepdim=True))
        alpha = torch.exp2(m - m_new) if rescale else torch.ones_like(m)
        e = torch.exp2(t - m_new)
        l = l * alpha + e.sum(-1, keepdim=True)
        acc = acc * alpha + rnd_p(e) @ v[j0:j0 + 64]
        m = m_new
    return acc / l


def _bias(relh, relw, b, h, Nk, S, swap, dt):
    j = torch.arange(Nk)
    jh, jw = (j % S, j // S) if swap else (j // S, j % S)
    return relh[b, h].to(dt)[:, jh.clamp_max(S - 1)] + relw[b, h].to(dt)[:, jw.clamp_max(S - 1)]


def attn_ref(q, k, v, scale, *, causal=False, q_pos0=0, relh=None, relw=None, S=0, nk_rows=None, **wrong):
    """-> out [B, H, Nq, d] float64. A row that sees no key (only under a mistake flag) is 0."""
    fl = dict.fromkeys(MISTAKES, False)
    assert set(wrong) <= set(MISTAKES), wrong
    fl.update(wrong)
    B, H, Nq, d = q.shape
    Nk = k.shape[2]
    vd = v.double()
    if fl["next_head_v"]:
        vd = vd.roll(-1, 1) if H > 1 else vd.roll(-1, 0)
    if fl["key_plus1"]:
        vd = vd[:, :, (torch.arange(Nk) + 1).clamp_max(Nk - 1)]
    out = torch.empty((B, H, Nq, d), dtype=F64)
    for b in range(B):
        nk = Nk if nk_rows is None else min(Nk, int(nk_rows[0 if fl["nk_of_batch0"] else b]) + (1 if fl["nk_plus1"] else 0))
        vis = _visible(Nq, Nk, nk, causal, q_pos0, fl)
        for h in range(H):
            s = (q[b, h].double() * f32(scale)) @ k[b, h].double().T
            if relh is not None:
                s = s + _bias(relh, relw, b, h, Nk, S, fl["swap_hw"], F64)
            s = torch.where(vis, s, torch.full_like(s, -INF))
            vv = torch.where(vis.any(0)[:, None], vd[b, h], torch.zeros_like(vd[b, h]))     # 0 * NaN: a row no query sees
            if fl["no_rescale"]:
                out[b, h] = _online(s * LOG2E, vv, F64, lambda x: x, rescale=False)
            else:
                out[b, h] = torch.nan_to_num(torch.softmax(s, -1), nan=0.0) @ vv
    return out


def attn_blocked(c, family):
    """The same result, correct, in fp32 with the kernels' documented roundings and no others, 64 keys at a time. 16-bit P.V
    kernels (generic, pp, window): Qs = r16(q * fp32(scale log2e)), bias * log2e added in fp32, r16(p) multiplies V, out = r16(acc /
    l). decode: q * fp32(scale log2e) unrounded, p fp32, out r16. f32: natural scores scaled to log2 in fp32, nothing rounded."""
    dt = c.q.dtype
    r16 = (lambda x: x.to(dt).float()) if dt != F32 else (lambda x: x)
    p16 = family in ("generic", "pp", "window") and dt != F32
    B, H, Nq, d = c.q.shape
    Nk = c.k.shape[2]
    fl = dict.fromkeys(MISTAKES, False)
    out = torch.empty((B, H, Nq, d), dtype=dt)
    for b in range(B):
        nk = Nk if c.nk_rows is None else int(c.nk_rows[b])
        vis = _visible(Nq, Nk, nk, c.causal, c.q_pos0, fl)
        for h in range(H):
            qs = c.q[b, h].float() * sl2(c.scale)
            qs = r16(qs) if p16 else qs
            if c.mates is None:
                s = qs @ c.k[b, h].float().T
            else:     # tied keys: every key's dot product in ONE order, as a kernel's lanes form it (a BLAS picks its order per column)
                s = (qs[:, None, :] * c.k[b, h].float()[None, :, :]).sum(-1)
            if c.relh is not None:
                s = s + _bias(c.relh, c.relw, b, h, Nk, c.S, False, F32) * np.float32(LOG2E)
            s = torch.where(vis, s, torch.full_like(s, -INF))
            vv = torch.where(vis.any(0)[:, None], c.v[b, h].float(), torch.zeros((), dtype=F32))
            out[b, h] = _online(s, vv, F32, r16 if p16 else (lambda x: x)).to(dt)
    return out


def scores2(c, b, h, rounded):
    """float64 scores of head (b, h) in log2 units, -inf where invisible, on the Q the kernels multiply K by: r16(q * fp32(scale
    log2e)) (rounded: the 16-bit MFMA kernels) or the unrounded product (decode, fp32) -> [Nq, Nk]"""
    Nq, Nk = c.q.shape[2], c.k.shape[2]
    qs = c.q[b, h].float() * sl2(c.scale)
    qs = (qs.to(c.q.dtype) if rounded else qs).double()
    nk = Nk if c.nk_rows is None else int(c.nk_rows[b])
    vis = _visible(Nq, Nk, nk, c.causal, c.q_pos0, dict.fromkeys(MISTAKES, False))
    t = qs @ c.k[b, h].double().T
    if c.relh is not None:
        t = t + _bias(c.relh, c.relw, b, h, Nk, c.S, False, F64) * LOG2E
    return torch.where(vis, t, torch.full_like(t, -INF))


def assert_margin(c):
    """the chosen key (and its mates) lead every other visible key by MARGIN log2 units; a late_jump key sits its gap +- JUMP_TOL below"""
    worst = INF
    B, H = c.q.shape[:2]
    for rounded in ((True, False) if c.q.dtype != F32 else (False,)):
        for b in range(B):
            for h in range(H):
                s = scores2(c, b, h, rounded)
                idx = c.choice[b, h][:, None]
                top = s.gather(-1, idx)
                assert bool(torch.isfinite(top).all()), "a chosen key is not visible"
                rest = s.scatter(-1, idx, -INF)
                if c.mates is not None:
                    mt = c.mates[b, h]
                    # (their K rows are the same bits; a BLAS picks its summation order per column, so float64 agrees to rounding)
                    assert bool((((s - top).abs() <= 1e-9 * top.abs()) | ~mt | torch.isinf(s)).all()), "mates do not tie with the chosen key"
                    rest = torch.where(mt, torch.full_like(s, -INF), rest)
                if c.jump is not None:
                    jx = c.jump[b, h][:, None]
                    sj = rest.gather(-1, jx)
                    seen = torch.isfinite(sj) & (jx != idx)
                    gap = (top - sj)[seen]
                    assert gap.numel() == 0 or (float(gap.min()) >= c.jump_gap - JUMP_TOL and float(gap.max()) <= c.jump_gap + JUMP_TOL), (float(gap.min()), float(gap.max()))
                    rest = torch.where(seen, rest.scatter(-1, jx, -INF), rest)
                lead = top - rest.amax(-1, keepdim=True)
                if c.is_pad is not None:      # a padded window position's query row is never compared
                    lead = lead[~c.is_pad[b]]
                worst = min(worst, float(lead.min()))
    assert worst >= MARGIN, f"margin {worst} < {MARGIN}"
    return worst


# ----------------------------------------------------------------------------------------------------------------- builders
def _nk_list(B, Nk, nk_rows):
    return [Nk] * B if nk_rows is None else [int(n) for n in nk_rows]


def _gather_rows(x, idx):
    """x [B,H,N,d], idx [B,H,M] -> [B,H,M,d]"""
    return x.gather(2, idx[..., None].expand(*idx.shape, x.shape[-1]))


def cycle_choice(Nq, nk, causal, q_pos0, shift=0):
    """keys 0, 63, 64, 127, 128, nk - 1 and the causal diagonal in turn; the diagonal (causal) or nk - 1 where the turn's key is not
    visible, and for the last query"""
    i = torch.arange(Nq)
    diag = torch.clamp(i + q_pos0, 0, nk - 1) if causal else torch.full((Nq,), nk - 1)
    cand = torch.tensor([0, 63, 64, 127, 128, nk - 1, -1])[(i + shift) % 7]
    choice = torch.where((cand < 0) | (cand > diag) | (cand >= nk), diag, cand)
    choice[-1] = diag[-1]
    return choice


def select_by_qk(B, H, Nq, Nk, d, seed, dtype, causal=False, q_pos0=0, nk_rows=None, choice=None, scale=None):
    k = unit_rows((B, H, Nk, d), seed, dtype, amp_of(d))
    v = rand((B, H, Nk, d), seed + 1).to(dtype)
    if choice is None:
        nks = _nk_list(B, Nk, nk_rows)
        choice = torch.stack([torch.stack([cycle_choice(Nq, nks[b], causal, q_pos0, b * H + h) for h in range(H)]) for b in range(B)])
    q = (GAIN * _gather_rows(k, choice).float()).to(dtype)
    c = Case(q=q, k=k, v=v, scale=d ** -0.5 if scale is None else scale, causal=causal, q_pos0=q_pos0, nk_rows=nk_rows, choice=choice)
    c.vmax = c.v_choice().abs()
    assert_margin(c)
    return c


def grid_choice(Nq, n_rows, S, shift=0):
    """(kh, kw) per query: the four grid corners, the last key of the row before the last (key 63 of tile nkt - 2 where S = 64), and
    the transposed position (i % S, (i // S) % n_rows), clamped: with it, swapped h / w or / S for % S picks another key"""
    i = torch.arange(Nq)
    t = (i + shift) % 6
    kh = torch.where(t == 0, 0, torch.where(t == 1, 0, torch.where(t == 2, n_rows - 1, torch.where(t == 3, n_rows - 1, torch.where(
        t == 4, max(n_rows - 2, 0), (i % S).clamp_max(n_rows - 1))))))
    kw = torch.where(t == 0, 0, torch.where(t == 1, S - 1, torch.where(t == 2, 0, torch.where(t == 3, S - 1, torch.where(
        t == 4, S - 1, ((i // S) % n_rows).clamp_max(S - 1))))))
    kh[-1], kw[-1] = n_rows - 1, S - 1      # the last key is chosen by the last query
    return kh, kw


def select_by_bias(B, H, Nq, Nk, d, S, seed, dtype):
    assert Nk % S == 0
    q, k = (rand((B, H, Nq, d), seed) * 0.5).to(dtype), (rand((B, H, Nk, d), seed + 1) * 0.5).to(dtype)
    v = rand((B, H, Nk, d), seed + 2).to(dtype)
    relh, relw = torch.zeros((B, H, Nq, S)), torch.zeros((B, H, Nq, S))
    choice = torch.empty((B, H, Nq), dtype=torch.long)
    for b in range(B):
        for h in range(H):
            kh, kw = grid_choice(Nq, Nk // S, S, 5 * (b * H + h))
            relh[b, h, torch.arange(Nq), kh] = BIAS_ON
            relw[b, h, torch.arange(Nq), kw] = BIAS_ON
            choice[b, h] = kh * S + kw
    c = Case(q=q, k=k, v=v, scale=d ** -0.5, relh=relh, relw=relw, S=S, choice=choice)
    c.vmax = c.v_choice().abs()
    assert_margin(c)
    return c


def relpos_from_tables(q, tab_h, tab_w, S, rel_row_plus1=False):
    """The decomposed bias of image_encoder.py:354-392 for q [B,H,S*S,d]: relh[q, kh] = q . tab_h[qy - kh + S - 1], relw[q, kw] = q .
    tab_w[qx - kw + S - 1], UNSCALED q, on the tables as given (already 16-bit values) -> fp32-exact float64 [B,H,N,S] pair"""
    idx = torch.arange(S)[:, None] - torch.arange(S)[None, :] + (S - 1) + (1 if rel_row_plus1 else 0)
    idx = idx.clamp(0, 2 * S - 2)
    B, H, N, d = q.shape
    rq = q.double().reshape(B, H, S, S, d)
    relh = torch.einsum("bhyxc,ykc->bhyxk", rq, tab_h.double()[idx]).reshape(B, H, N, S)
    relw = torch.einsum("bhyxc,xkc->bhyxk", rq, tab_w.double()[idx]).reshape(B, H, N, S)
    return relh, relw


def window_fill(qkv, grid, S, pad_row, pad_as_zero=False):
    """qkv [n_win, S*S, 3, H, d], windows tiling images of grid x grid tokens, wps = ceil(grid / S) a side: the pad token's q / k / v
    (pad_row [3, H, d]) written into every padded position, which is what window_partition's zero pad plus the qkv bias produces.
    -> (filled copy, is_pad [n_win, S*S])"""
    n_win = qkv.shape[0]
    wps = -(-grid // S)
    is_pad = torch.zeros((n_win, S, S), dtype=torch.bool)
    for w in range(n_win):
        wy, wx = (w % (wps * wps)) // wps, (w % (wps * wps)) % wps
        is_pad[w, max(0, grid - wy * S):, :] = True
        is_pad[w, :, max(0, grid - wx * S):] = True
    is_pad = is_pad.view(n_win, S * S)
    full = qkv.clone()
    full[is_pad] = torch.zeros_like(pad_row) if pad_as_zero else pad_row
    return full, is_pad


WIN_S, WIN_D = 14, 80


def _window_case(qkv, pad_row, grid, choice, tab_h, tab_w, dtype, **wrong):
    """the Case of the FILLED windows; wrong: pad_as_zero, rel_row_plus1"""
    full, is_pad = window_fill(qkv, grid, WIN_S, pad_row, wrong.get("pad_as_zero", False)) if grid else (qkv, torch.zeros(qkv.shape[:2], dtype=torch.bool))
    q, k, v = (full[:, :, i].permute(0, 2, 1, 3).unsqueeze(0)[0] for i in range(3))     # [n_win, H, N, d]
    relh, relw = relpos_from_tables(q, tab_h, tab_w, WIN_S, wrong.get("rel_row_plus1", False))
    c = Case(q=q, k=k, v=v, scale=WIN_D ** -0.5, relh=relh.float(), relw=relw.float(), S=WIN_S, choice=choice, grid=grid, is_pad=is_pad,
             tab_h=tab_h, tab_w=tab_w, qkv=qkv, pad_row=pad_row)
    assert torch.equal(c.relh.double(), relh) and torch.equal(c.relw.double(), relw)     # the builders' biases are exact in fp32
    return c


def _finish_window(c):
    n_win, H, N, _ = c.q.shape
    pad_k = c.is_pad[:, None, None, :].expand(n_win, H, N, N)
    chosen_pad = c.is_pad.gather(1, c.choice.reshape(n_win, -1)).reshape(n_win, H, N, 1)
    c.mates = pad_k & chosen_pad           # every padded position holds the pad token: they tie, and share one V row
    if not bool(c.mates.any()):
        c.mates = None
    c.vmax = c.v_choice().abs()
    c.real = ~c.is_pad
    return c


def window_choice(n_win, H):
    ch = torch.empty((n_win, H, WIN_S * WIN_S), dtype=torch.long)
    for w in range(n_win):
        for h in range(H):
            kh, kw = grid_choice(WIN_S * WIN_S, WIN_S, WIN_S, w * H + h)
            ch[w, h] = kh * WIN_S + kw
    return ch


def select_by_tables_14(n_win, H, seed, dtype, grid=0, **wrong):
    """tab_h[r] = 12 e_r on dims 0..26, tab_w[r] = 12 e_(27 + r); q_i = 12 (e_a + e_(27 + b)), a = qy - kh* + 13, b = qx - kw* + 13;
    k = 0 (the pad token's too): the bias is 144 ([kh == kh*] + [kw == kw*]); every value is exact in bf16 and f16"""
    S, d, N = WIN_S, WIN_D, WIN_S * WIN_S
    tab_h, tab_w = torch.zeros((2 * S - 1, d)), torch.zeros((2 * S - 1, d))
    tab_h[torch.arange(27), torch.arange(27)] = 12.0
    tab_w[torch.arange(27), 27 + torch.arange(27)] = 12.0
    choice = window_choice(n_win, H)
    qy, qx = torch.arange(N) // S, torch.arange(N) % S
    qkv = torch.zeros((n_win, N, 3, H, d))
    qkv[:, :, 2] = rand((n_win, N, H, d), seed)
    for h in range(H):
        a, b = qy - choice[:, h] // S + 13, qx - choice[:, h] % S + 13      # [n_win, N]
        qkv[:, :, 0, h].scatter_(-1, a[..., None], 12.0)
        qkv[:, :, 0, h].scatter_(-1, 27 + b[..., None], 12.0)
    pad_row = torch.zeros((3, H, d))
    pad_row[2] = rand((H, d), seed + 1)
    pad_row[0] = rand((H, d), seed + 2)
    c = _window_case(qkv.to(dtype), pad_row.to(dtype), grid, choice, tab_h.to(dtype), tab_w.to(dtype), dtype, **wrong)
    c = _finish_window(c)
    if c.mates is not None:     # bias-selected: a padded position is told from the other pads by its bias, nothing ties
        c.mates = None
    if not wrong:
        assert_margin(c)
    return c


def select_window_qk(n_win, H, seed, dtype, grid=0, **wrong):
    """select_by_qk on the window geometry with zero tables; every (window, head) has its own K / V"""
    S, d, N = WIN_S, WIN_D, WIN_S * WIN_S
    choice = window_choice(n_win, H)
    qkv = torch.empty((n_win, N, 3, H, d), dtype=dtype)
    qkv[:, :, 1] = unit_rows((n_win, N, H, d), seed, dtype, amp_of(d))
    qkv[:, :, 2] = rand((n_win, N, H, d), seed + 1).to(dtype)
    pad_row = torch.stack([rand((H, d), seed + 2).to(dtype), unit_rows((H, d), seed + 3, dtype, amp_of(d)), rand((H, d), seed + 4).to(dtype)])
    full, _ = window_fill(qkv, grid, S, pad_row) if grid else (qkv, None)
    kf = full[:, :, 1].permute(0, 2, 1, 3)
    qkv[:, :, 0] = (GAIN * _gather_rows(kf, choice).float()).to(dtype).permute(0, 2, 1, 3)
    zero = torch.zeros((2 * S - 1, d), dtype=dtype)
    c = _finish_window(_window_case(qkv, pad_row, grid, choice, zero, zero, dtype, **wrong))
    if not wrong:
        assert_margin(c)
    return c


GLB_S, GLB_D = 64, 80


def select_by_tables_64(H, seed, dtype, tables_seed=6):
    """fused global kernel (N = 4096, d = 80, 127 table rows): tab_h[r] = 3 s_r on dims 0..39, tab_w[r] = 3 s'_r on dims 40..79, s in
    {+-1}^40; q_i = 3 (s_a | s'_b), k = 0. The bias is 9 (s_a . s_r + s'_b . s'_r'): 720 for the chosen key, at most 360 + 9 * 20 for
    any other as long as the largest off-diagonal dot product is 20 of 40 (asserted)."""
    S, d, N = GLB_S, GLB_D, GLB_S * GLB_S
    sh, sw = (torch.randint(0, 2, (2 * S - 1, 40), generator=torch.Generator(device="cpu").manual_seed(sd)).float() * 2 - 1
              for sd in (tables_seed, tables_seed + 10))      # seeds 6 and 16: the first two that meet the assertion below
    for s in (sh, sw):
        off = (s @ s.T - 40 * torch.eye(2 * S - 1)).amax()
        assert float(off) <= 20, float(off)
    tab_h, tab_w = torch.zeros((2 * S - 1, d)), torch.zeros((2 * S - 1, d))
    tab_h[:, :40], tab_w[:, 40:] = 3 * sh, 3 * sw
    choice = torch.empty((1, H, N), dtype=torch.long)
    q = torch.empty((1, H, N, d))
    qy, qx = torch.arange(N) // S, torch.arange(N) % S
    for h in range(H):
        kh, kw = grid_choice(N, S, S, 7 * h)
        choice[0, h] = kh * S + kw
        q[0, h, :, :40], q[0, h, :, 40:] = 3 * sh[qy - kh + S - 1], 3 * sw[qx - kw + S - 1]
    k = torch.zeros((1, H, N, d), dtype=dtype)
    v = rand((1, H, N, d), seed).to(dtype)
    q, tab_h, tab_w = q.to(dtype), tab_h.to(dtype), tab_w.to(dtype)
    relh, relw = relpos_from_tables(q, tab_h, tab_w, S)
    c = Case(q=q, k=k, v=v, scale=d ** -0.5, relh=relh.float(), relw=relw.float(), S=S, choice=choice, tab_h=tab_h, tab_w=tab_w)
    assert torch.equal(c.relh.double(), relh)
    c.vmax = c.v_choice().abs()
    assert_margin(c)
    return c


def recast_tables_64(c, dtype):
    """a select_by_tables_64 case in the other 16-bit type: q and the tables hold 0 and +-3, exact in both, so the scores and the
    margin asserted at construction are the same; v is re-rounded and is the reference's v"""
    if dtype == c.q.dtype:
        return c
    f = Case(**{**c.__dict__, **{n: getattr(c, n).to(dtype) for n in ("q", "k", "v", "tab_h", "tab_w")}})
    assert torch.equal(f.q.float(), c.q.float()) and torch.equal(f.tab_h.float(), c.tab_h.float()) and torch.equal(f.tab_w.float(), c.tab_w.float())
    f.vmax = f.v_choice().abs()
    return f


def heads_of(c, H):
    """the first H heads of a case, as a case of its own"""
    names = [n for n in ("q", "k", "v", "choice", "vmax", "relh", "relw") if getattr(c, n, None) is not None]
    return Case(**{**c.__dict__, **{n: getattr(c, n)[:, :H] for n in names}})


def pair_inputs(B, H, Nq, Nk, d, seed, dtype, causal=False, q_pos0=0, nk_rows=None, late_jump=False, first=16, S=0):
    """Per (batch, head) two keys a < b with k[b] = k[a] bit for bit and q = GAIN * k[a] for every query: the two scores are equal in
    any accumulation order and out = (v[a] + v[b]) / 2. a = (3 h + b) % min(first, nk[, q_pos0 + 1]) lies in the first key tile /
    wave trip / row group, b = nk - 1 is the last key. A causal query that does not see b answers v[a]. late_jump (True: JUMP, or
    the gap in log2 units): key 0 holds (1 - gap / top) k[a] and a moves to key 64 + (a % 16) (key 1 + ... where nk <= 81): tile 0's maximum is JUMP log2 units below
    the pair, which arrives later. S > 0: zero fp32 rel-pos terms ride along (the kernels that only run with a bias)."""
    nks = _nk_list(B, Nk, nk_rows)
    gap = JUMP if late_jump is True else float(late_jump)
    k = unit_rows((B, H, Nk, d), seed, dtype, amp_of(d))
    v = rand((B, H, Nk, d), seed + 1).to(dtype)
    scale = d ** -0.5
    A = torch.empty((B, H), dtype=torch.long)
    Bk = torch.empty((B, H), dtype=torch.long)
    J = torch.zeros((B, H), dtype=torch.long)
    for b in range(B):
        for h in range(H):
            a = (3 * h + b) % min(first, nks[b], q_pos0 + 1 if causal else nks[b])
            if late_jump and nks[b] >= 4:
                a = (64 + a % 16) if nks[b] > 81 else 1 + a % (nks[b] - 2)
                top = GAIN * float((k[b, h, a].double() ** 2).sum()) * sl2(scale)
                k[b, h, 0] = (k[b, h, a].double() * (1.0 - gap / top)).to(dtype)
            A[b, h], Bk[b, h] = a, nks[b] - 1
            k[b, h, nks[b] - 1] = k[b, h, a]
    q = (GAIN * _gather_rows(k, A[..., None]).float()).to(dtype).expand(B, H, Nq, d).contiguous()
    i = torch.arange(Nq)
    sees_b = (Bk[..., None] <= i + q_pos0) if causal else torch.ones((B, H, Nq), dtype=torch.bool)
    sees_a = (A[..., None] <= i + q_pos0) if causal else torch.ones((B, H, Nq), dtype=torch.bool)
    choice = torch.where(sees_a, A[..., None].expand(B, H, Nq), J[..., None].expand(B, H, Nq))
    j = torch.arange(Nk)
    mates = (j == Bk[..., None, None]) & sees_b[..., None] & (Bk != A)[..., None, None]
    c = Case(q=q, k=k, v=v, scale=scale, causal=causal, q_pos0=q_pos0, nk_rows=nk_rows, choice=choice, mates=mates.expand(B, H, Nq, Nk),
             onehot=False, jump=J[..., None].expand(B, H, Nq).contiguous() if late_jump else None, pair=(A, Bk), jump_gap=gap)
    va, vb, vj = _gather_rows(v, choice).abs(), _gather_rows(v, Bk[..., None].expand(B, H, Nq)).abs(), _gather_rows(v, c.jump).abs() if late_jump else 0
    c.vmax = torch.maximum(torch.maximum(va, vb), vj) if late_jump else torch.maximum(va, vb)
    if S:
        c.S, c.relh, c.relw = S, torch.zeros((B, H, Nq, S)), torch.zeros((B, H, Nq, S))
    assert_margin(c)
    return c


def ragged_poison(c, nan=False):
    """rows >= nk_rows[b] of the cache: K = 2 * k[choice of query 0], V = 1000 (finite: they would win if seen), or NaN"""
    B, H, _, d = c.q.shape
    for b in range(B):
        n = int(c.nk_rows[b])
        if nan:
            c.k[b, :, n:], c.v[b, :, n:] = NAN, NAN
        else:
            c.k[b, :, n:] = (2.0 * _gather_rows(c.k, c.choice[:, :, :1])[b].float()).to(c.k.dtype)
            c.v[b, :, n:] = 1000.0
    return c


# --------------------------------------------------------------------------------------------------------------------- RoPE
def cos_sin_table(Tmax, d, theta=10000.0):
    """fp32 [Tmax, d] = cos(0..d/2) | sin(0..d/2), as the model builds it"""
    inv = 1.0 / (theta ** (torch.arange(0, d, 2, dtype=F32) / d))
    ang = torch.arange(Tmax, dtype=F32)[:, None] * inv[None, :]
    return torch.cat([ang.cos(), ang.sin()], 1).contiguous()


def rope(x, pos, cos_sin, inverse=False):
    """rotate-half RoPE in float64: x [..., d] at positions pos (broadcast against x's leading dims)"""
    d = x.shape[-1]
    cs = cos_sin.double()[pos]
    c, s = cs[..., :d // 2], cs[..., d // 2:]
    if inverse:
        s = -s
    x1, x2 = x.double()[..., :d // 2], x.double()[..., d // 2:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)


def rope_inv(x, pos, cos_sin):
    return rope(x, pos, cos_sin, inverse=True)


DEC_D = 128


def decode_choice(B, H, nks):
    """(7 h + b) % nk, forced to the last key for h = 0 and to key 0 for h = 1"""
    ch = torch.empty((B, H, 1), dtype=torch.long)
    for b in range(B):
        for h in range(H):
            ch[b, h, 0] = nks[b] - 1 if h == 0 else (0 if h == 1 else (7 * h + b) % nks[b])
    return ch


def decode_case(B, H, Tmax, nks, seed, dtype, pair=False, nan=False):
    if pair:
        c = pair_inputs(B, H, 1, Tmax, DEC_D, seed, dtype, nk_rows=nks)
    else:
        c = select_by_qk(B, H, 1, Tmax, DEC_D, seed, dtype, nk_rows=nks, choice=decode_choice(B, H, nks))
    return ragged_poison(c, nan)


def chain_choice(B, H, nks, shift=0):
    """The chained decode step's attention stage (one workgroup per (row, head), four waves that take every fourth trip of 16 keys,
    256 keys requested before the wait): (row, head) pair i takes turn (i + shift) % 10 of key 0, the new row nk - 1, the last cached
    row nk - 2, keys 16, 32 and 48 (the first key of waves 1 to 3), keys 255, 256, 257 (both sides of the pre-wait registers) and
    300; a turn whose key the row does not see passes to the next one (key 0 is always seen)."""
    ch = torch.empty((B, H, 1), dtype=torch.long)
    for b in range(B):
        cand = [0, nks[b] - 1, nks[b] - 2, 16, 32, 48, 255, 256, 257, 300]
        for h in range(H):
            t = (b * H + h + shift) % len(cand)
            while not 0 <= cand[t] < nks[b]:
                t = (t + 1) % len(cand)
            ch[b, h, 0] = cand[t]
    return ch


def rope_case(B, H, Tmax, nks, seed, dtype, choice=None):
    """The fused-RoPE decode step: -> (Case of the ROTATED problem (what the kernel attends), qkv_raw [B, 3, H, d], caches before the
    step k0, v0 [B,H,Tmax,d] with NaN from row nk - 1 on, cos_sin). q_raw = r16(rope_inv(GAIN * kcache[choice])) for an old key,
    GAIN * k_new for the new row; the Case's q is r16(rope(q_raw)), its k row nk - 1 is r16(rope(k_new)). choice [B, H, 1]: the key
    every (row, head) answers with (default: decode_choice)."""
    d = DEC_D
    cs = cos_sin_table(Tmax, d)
    pos = torch.tensor([n - 1 for n in nks])
    k = unit_rows((B, H, Tmax, d), seed, dtype, amp_of(d))
    v = rand((B, H, Tmax, d), seed + 1).to(dtype)
    k_new = unit_rows((B, H, d), seed + 2, dtype, amp_of(d))
    v_new = rand((B, H, d), seed + 3).to(dtype)
    choice = decode_choice(B, H, nks) if choice is None else choice
    rot = lambda x: rope(x, pos[:, None], cs).to(dtype)   # noqa: E731
    k_rot = rot(k_new)
    is_new = choice[..., 0] == pos[:, None]
    q_old = rope_inv(GAIN * _gather_rows(k, choice)[:, :, 0].double(), pos[:, None], cs).to(dtype)
    q_raw = torch.where(is_new[..., None], (GAIN * k_new.float()).to(dtype), q_old)
    k0, v0 = k.clone(), v.clone()
    for b in range(B):
        k0[b, :, nks[b] - 1:], v0[b, :, nks[b] - 1:] = NAN, NAN
        k[b, :, nks[b] - 1], v[b, :, nks[b] - 1] = k_rot[b], v_new[b]
    c = Case(q=rot(q_raw)[:, :, None], k=k, v=v, scale=d ** -0.5, nk_rows=nks, choice=choice)
    c.vmax = c.v_choice().abs()
    assert_margin(c)
    c.k_rot64 = rope(k_new, pos[:, None], cs)
    ragged_poison(c, nan=True)
    return c, torch.stack([q_raw, k_new, v_new], 1), k0, v0, cs


# --------------------------------------------------------------------------------------------------------------- case lists
# generic kernel, no bias: (d, B, H, Nq, Nk, causal, q_pos0). dp 64 at d = 64, dp 96 at d = 72 (d % 16 != 0) and 80, dp 128 at d = 104
GENERIC_NK = ((1, 1), (63, 64), (65, 63), (128, 127), (129, 129), (130, 70))
GENERIC_PLAIN = tuple((d, 1, 1, nq, nk, 0, 0) for d in (64, 72, 80, 104) for nq, nk in GENERIC_NK) + (
    (64, 1, 1, 70, 133, 1, 10), (64, 1, 2, 70, 133, 1, 63),        # causal: 0 < q_pos0 < Nk - Nq, q_pos0 = Nk - Nq
    (64, 1, 3, 129, 129, 0, 0), (80, 2, 4, 130, 70, 0, 0),         # grid decodes: B * H = 3 (id / nqb) and 8 with nqb = 2
    (64, 2, 4, 129, 129, 1, 0))
# generic kernel, fp32 rel-pos terms: (d, B, H, Nq, Nk, S) and the branch of attention_bf16_impl each reaches
GENERIC_BIAS3 = tuple((d, 1, 2, S * S, S * S, S) for S in (7, 14, 16) for d in (32, 80))
GENERIC_BIAS1 = tuple((d, 1, 2, nq, nk, S) for S, nk in ((3, 6), (14, 182), (20, 400), (32, 1024)) for nq in (5, 130) for d in ((64, 80) if S == 14 else (64,)))
GENERIC_BIAS2 = ((64, 1, 2, 130, 128, 64), (64, 1, 1, 5, 320, 64), (128, 1, 1, 130, 128, 64), (128, 1, 2, 5, 320, 64),
                 (80, 1, 2, 128, 320, 64),       # FULL + LSUM
                 (80, 1, 2, 100, 128, 64))       # LSUM, not FULL
# separate k and v tensors, v at the LOWER address: attn_global_pp_ok asks for equal strides, v >= k, a span below 2^31 bytes and
# 16-byte alignment (not for one allocation), so it is the pointer order that turns the ping-pong kernel away -> FULL + LSUM
GENERIC_BIAS2_SPLIT_KV = (80, 1, 2, 256, 128, 64)
RAGGED_NK = (1, 63, 64, 65, 130)                   # through attention_decode_rows at d = 64: Tmax = 130, B = 5, H = 3
# ping-pong kernel, fp32 tables: (B, H, Nq, nkt)
PP_TABLES = tuple((1, 3, 256, nkt) for nkt in range(2, 10)) + ((2, 4, 512, 5), (1, 3, 512, 9))
PP_PAIR = ((1, 3, 256, 5, False), (2, 4, 512, 4, False), (1, 3, 256, 5, True), (2, 4, 512, 9, True),    # (B, H, Nq, nkt, late_jump)
           (1, 3, 256, 5, JUMP_CLEAR), (2, 4, 512, 9, JUMP_CLEAR))
PP_FUSED_H = (1, 3)
# decode kernels (d = 128): (B, H, Tmax, nk_rows)
NK300 = (1, 2, 4, 5, 15, 16, 17, 63, 64, 65, 255, 256, 257, 300)
NK70 = (1, 3, 4, 5, 16, 17, 33, 64, 65, 70, 2, 63, 69)
DECODE = ((14, 2, 300, NK300),        # B * H = 28 <= 128: 16 waves share a pair
          (14, 16, 300, NK300),       # 224 <= 1024: 4 waves, a round is 64 keys
          (13, 81, 70, NK70))         # 1053 > 1024, odd: one wave per head, the last workgroup has one live wave
# window kernel: (n_win, H) without padding; (grid, H) with two images per launch
WINDOW_ITEMS = ((1, 1), (7, 1), (8, 1), (85, 3), (64, 4), (257, 1), (90, 3))
WINDOW_GRIDS = tuple((g, H) for g in (14, 15, 20, 28) for H in (1, 3))
# fp32 kernels: (d, B, H, Nq, Nk, causal, q_pos0, S)
F32_NK = ((1, 1), (3, 17), (4, 16), (5, 300))
F32_PLAIN = tuple((d, 1, 2, nq, nk, 0, 0, 0) for d in (16, 80, 256) for nq, nk in F32_NK) + tuple(
    (d, 2, 1, nq, nk, 1, p0, 0) for d in (16, 80) for nq, nk in F32_NK[1:] for p0 in (0, nk - nq))
F32_FEW = tuple((d, 1, 2, nq, nk, 0, 0, 0) for d in (16, 32) for nq in (256, 257) for nk in (1, 16))
F32_BIAS = ((16, 1, 2, 5, 49, 0, 0, 7), (80, 1, 1, 3, 128, 0, 0, 64), (80, 1, 2, 49, 49, 1, 0, 7), (16, 1, 1, 70, 128, 1, 58, 64))
F32_RAGGED = ((16, 5, 2, 17, (1, 2, 16, 17, 9)), (80, 4, 3, 300, (1, 64, 257, 300)))      # (d, B, H, Tmax, nk_rows)


def case_id(t):
    return "-".join(str(x) for x in t if not isinstance(x, tuple))


def causal_bias_case(d, B, H, Nq, Nk, q_pos0, S, seed, dtype):
    """fp32 entry point only: rel-pos terms together with the causal mask. Every query's bias points at a key it sees: the diagonal's
    (kh, kw) for even queries, key 0 for odd ones"""
    c = select_by_bias(B, H, Nq, Nk, d, S, seed, dtype)
    i = torch.arange(Nq)
    key = torch.where(i % 2 == 0, (i + q_pos0).clamp_max(Nk - 1), torch.zeros_like(i))
    c.relh.zero_()
    c.relw.zero_()
    c.relh[:, :, i, key // S] = BIAS_ON
    c.relw[:, :, i, key % S] = BIAS_ON
    c.choice = key.expand(B, H, Nq).contiguous()
    c.causal, c.q_pos0 = True, q_pos0
    c.vmax = c.v_choice().abs()
    assert_margin(c)
    return c
