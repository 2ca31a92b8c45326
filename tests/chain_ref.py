"""Plain CPU restatement of the chained decode step (haff_decode_chain_bf16, csrc/decode_chain.hip), written from the entry point's
documentation: per layer

  stage 0  qkv   = r16(rstd_in[m] * (x . wqkv^T))            wqkv [3H, H] carries input_layernorm's gamma in its columns; rstd_in is
                                                               stats0[m, 1] on layer 0 and rsqrt(sum_p ssq_b[p, m] / H + eps) after it
  stage 1  q, k  = r16(rope(q | k at position nk_rows[m] - 1)) rotate-half on every 128-wide head, cos_sin = cos(64) | sin(64)
           cache rows nk_rows[m] - 1 of the layer's K / V cache <- k, v (v as stage 0 stored it)
           att   = r16(softmax(scale q . K^T) V)               over cache rows 0 .. nk_rows[m] - 1, the appended row included
  stage 2  x     = r16(att . wo^T + x)                         ssq_a[p, m] = sum of the ROUNDED x[m, 16 p : 16 p + 16] squared
  stage 3  g     = r16(silu(gate) * up)                        (gate | up) = rsqrt(sum_p ssq_a[p, m] / H + eps) * (x . wgu^T), wgu [2F, H]
                                                               in 16-row [gate | up] groups with post_attention_layernorm's gamma folded
  stage 4  x     = r16(g . wd^T + x)                           ssq_b likewise

r16 rounds to bf16 (every hand-off the kernel stores as bf16); round_handoffs=False leaves all of it out, and the step is then a
textbook Llama decoder layer (tests/test_chain_ref_cpu.py). Every stage is a function of tensors of its own, so a test can feed it
what the device handed on (teacher forcing); decode_chain_ref composes them. `dt` is torch.float64 for the reference and
torch.float32 for the same formula in fp32, whose distance from float64 the bounds are built from (train_edge_ref.bound).

Keyword flags switch on one deliberate mistake each (MISTAKES). The fixture builders and the checks of
tests/test_chain_edge_kernels_gpu.py live here too, so that tests/test_chain_ref_cpu.py can run the very same checks on this
restatement with a flag switched on and see them fail. Nothing here imports the package or touches a GPU."""
import torch

import attn_edge_ref as A
import gemm_edge_ref as G
import train_edge_ref as T

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64
NAN = float("nan")
D = 128
EPS = T.f32(1e-5)
SCALE = D ** -0.5
TMAX = 330

MISTAKES = ("drop_last_cached_key",    # cache row nk - 2 invisible
            "new_row_from_cache",      # row nk - 1 read from the cache (not yet written) instead of from qkv
            "rope_sign",               # the rotation partner enters with the other sign
            "cos_sin_swapped",         # the table's halves taken as sin | cos
            "k_half_wrong_tile",       # o_proj / down_proj: tile t adds the second K half of tile t + 1
            "ssq_exchanged",           # gate|up reads ssq_b, the next layer's q|k|v reads ssq_a
            "stats0_reused",           # stats0 on every layer
            "gate_up_swapped")         # silu(up) * gate

# the smallest geometries the entry point admits and one step up: (hidden, heads, ffn)
GEOMS = ((256, 2, 256),      # kq = 32 in o_proj / down_proj (one MFMA per wave), 64 in q|k|v and gate|up
         (256, 2, 512),      # config.mid()
         (512, 4, 768))
# nk_rows per launch: both sides of the 4-, 16-, 64- and 256-key edges, the empty cache, tmax itself
NK_GROUPS = ((1,), (2, 3, 4), (1, 2, 3, 4, 5, 15, 16, 17), (63, 64, 65, 255, 256, 257, 258, 319), (320, 321, 330, 1, 17))
NK_FOUR = (2, 16, 257, 329)      # at 2 heads: an attention stage of exactly 8 workgroups, the shard count
NK_MORE = ((17, 256), (1, 2, 3, 4, 5, 15), (63, 64, 65, 255, 256, 257, 258))      # M = 2, 6, 7: with the above every M of 1 .. 8


def onehot_cases():
    return [(g, nks) for g in GEOMS for nks in NK_GROUPS + ((NK_FOUR,) if g[1] == 2 else ())]


def dense_cases():
    return [(g, nks) for g in GEOMS for nks in NK_GROUPS + (NK_FOUR,) + NK_MORE]


def prefix_cases():
    return [(g, nks) for g in GEOMS for nks in (NK_GROUPS[4], NK_GROUPS[3])]


def case_id(t):
    (hidden, heads, ffn), nks = t
    return f"{hidden}x{heads}x{ffn}-M{len(nks)}-nk{nks[0]}"


def attn_workgroups():
    return sorted({len(nks) * g[1] for g, nks in onehot_cases()})


def r16(x, on=True):
    """one rounding to bf16 (through fp32, as the kernel's epilogues do), back in x's dtype"""
    return G.to16(x.double(), BF16).to(x.dtype) if on else x


# ------------------------------------------------------------------------------------------------------------------ stages
def ssq_groups(x):
    """sums of squares of x [M, H] over groups of 16 columns -> [H / 16, M] (the buffer's rows m < M)"""
    M, H = x.shape
    return (x * x).view(M, H // 16, 16).sum(-1).T.contiguous()


def rstd_of_ssq(ssq, M, K, eps=EPS, dt=F64):
    """ssq [K / 16, >= M] -> rsqrt(sum_p ssq[p, m] / K + eps) [M]"""
    return 1.0 / torch.sqrt(ssq.to(dt)[:, :M].sum(0) / K + torch.tensor(eps, dtype=dt))


def stage_qkv(x, wqkv, rstd, rnd=True, dt=F64):
    return r16(rstd.to(dt)[:, None] * (x.to(dt) @ wqkv.to(dt).T), rnd)


def rope_rows(x, pos, cos_sin, rope_sign=False, cos_sin_swapped=False):
    """x [M, heads, 128] at positions pos [M]: (x1 c - x2 s | x2 c + x1 s) on the halves of every head"""
    cs = cos_sin.to(x.dtype)[pos]
    c, s = cs[:, None, :D // 2], cs[:, None, D // 2:]
    if cos_sin_swapped:
        c, s = s, c
    if rope_sign:
        s = -s
    x1, x2 = x[..., :D // 2], x[..., D // 2:]
    return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1)


def stage_attention(qkv, kc, vc, cos_sin, nk_rows, heads, scale=SCALE, rnd=True, k_row=None, **wrong):
    """qkv [M, 3H]; kc, vc [M, tmax, H]: the caches BEFORE the step -> dict(q_rot, k_rot [M, H], att [M, H], att_unrounded (att before its
    own rounding), vmax [M, H]: the largest |v| among the rows att is made of, kc, vc: the caches after the step), float64. k_row [M, H]: the appended K row to attend
    (the one the device stored) in place of this function's own."""
    fl = dict.fromkeys(MISTAKES, False)
    assert set(wrong) <= set(MISTAKES), wrong
    fl.update(wrong)
    M, H = qkv.shape[0], heads * D
    q, k, v = (qkv.double()[:, i * H:(i + 1) * H].reshape(M, heads, D) for i in range(3))
    pos = torch.tensor([int(n) - 1 for n in nk_rows])
    rot = lambda t: r16(rope_rows(t, pos, cos_sin, fl["rope_sign"], fl["cos_sin_swapped"]), rnd)   # noqa: E731
    q_rot, k_rot = rot(q), rot(k)
    k_att = k_rot if k_row is None else k_row.double().reshape(M, heads, D)
    kc2, vc2 = kc.double().clone(), vc.double().clone()
    att, vmax = torch.empty((M, heads, D), dtype=F64), torch.empty((M, heads, D), dtype=F64)
    for b in range(M):
        n = int(nk_rows[b])
        K, V = kc2[b, :n].reshape(n, heads, D).clone(), vc2[b, :n].reshape(n, heads, D).clone()
        if not fl["new_row_from_cache"]:
            K[n - 1], V[n - 1] = k_att[b], v[b]
        vis = torch.ones(n, dtype=torch.bool)
        if fl["drop_last_cached_key"] and n >= 2:
            vis[n - 2] = False
        K, V = K[vis], V[vis]
        s = torch.einsum("hd,nhd->hn", q_rot[b], K) * T.f32(scale)
        att[b] = torch.einsum("hn,nhd->hd", torch.softmax(s, -1), V)
        vmax[b] = V.abs().amax(0)
        kc2[b, n - 1], vc2[b, n - 1] = k_rot[b].reshape(H), v[b].reshape(H)
    att = att.reshape(M, H)
    return dict(q_rot=q_rot.reshape(M, H), k_rot=k_rot.reshape(M, H), att=r16(att, rnd), att_unrounded=att, vmax=vmax.reshape(M, H), kc=kc2, vc=vc2)


def _halves(a, w, wrong_tile):
    """a . w^T as the sum of its two K halves per 16-column tile"""
    M, K = a.shape
    N = w.shape[0]
    p0, p1 = a[:, :K // 2] @ w[:, :K // 2].T, a[:, K // 2:] @ w[:, K // 2:].T
    if wrong_tile:
        p1 = p1.view(M, N // 16, 16).roll(-1, 1).reshape(M, N)
    return p0 + p1


def stage_resid(a, w, x, rnd=True, dt=F64, **wrong):
    """o_proj (a = att, w = wo) and down_proj (a = g, w = wd): -> (r16(a . w^T + x), its sums of squares [H / 16, M])"""
    y = r16(_halves(a.to(dt), w.to(dt), wrong.get("k_half_wrong_tile", False)) + x.to(dt), rnd)
    return y, ssq_groups(y)


stage_oproj = stage_down = stage_resid


def gate_up_pre(x, wgu, rstd, dt=F64, **wrong):
    """-> (gate, up) [M, F], the pre-activations"""
    M = x.shape[0]
    y = (rstd.to(dt)[:, None] * (x.to(dt) @ wgu.to(dt).T)).view(M, -1, 2, 16)
    gate, up = y[:, :, 0].reshape(M, -1), y[:, :, 1].reshape(M, -1)
    return (up, gate) if wrong.get("gate_up_swapped", False) else (gate, up)


def stage_gate_up(x, wgu, rstd, rnd=True, dt=F64, **wrong):
    gate, up = gate_up_pre(x, wgu, rstd, dt, **wrong)
    return r16(gate * torch.sigmoid(gate) * up, rnd)


def decode_chain_ref(layers, x, stats0, cos_sin, nk_rows, heads, eps=EPS, scale=SCALE, round_handoffs=True, ssq_fill=NAN, **wrong):
    """layers: (wqkv, wo, wgu, wd, kcache, vcache) per layer, the caches [M, tmax, H] before the step -> one dict per layer with every
    intermediate: qkv, q_rot, k_rot, att, kc, vc (after the step), x1, ssq_a, g, x2, ssq_b. ssq_fill: what ssq_b holds before the
    launch (only the `ssq_exchanged` mistake reads it)."""
    fl = dict.fromkeys(MISTAKES, False)
    assert set(wrong) <= set(MISTAKES), wrong
    fl.update(wrong)
    rnd = round_handoffs
    M, H = x.shape
    x = x.double()
    ssq_a = ssq_b = torch.full((H // 16, M), ssq_fill, dtype=F64)
    out = []
    for li, (wqkv, wo, wgu, wd, kc, vc) in enumerate(layers):
        if li == 0 or fl["stats0_reused"]:
            rstd = stats0.double()[:, 1]
        else:
            rstd = rstd_of_ssq(ssq_a if fl["ssq_exchanged"] else ssq_b, M, H, eps)
        r = dict(qkv=stage_qkv(x, wqkv, rstd, rnd))
        r.update(stage_attention(r["qkv"], kc, vc, cos_sin, nk_rows, heads, scale, rnd, **wrong))
        r["x1"], ssq_a = stage_oproj(r["att"], wo, x, rnd, **wrong)
        r["ssq_a"] = ssq_a
        r["g"] = stage_gate_up(r["x1"], wgu, rstd_of_ssq(ssq_b if fl["ssq_exchanged"] else ssq_a, M, H, eps), rnd, **wrong)
        r["x2"], ssq_b = stage_down(r["g"], wd, r["x1"], rnd, **wrong)
        r["ssq_b"] = ssq_b
        x = r["x2"]
        out.append(r)
    return out


def as_launch(res):
    """what an n-layer launch leaves behind, from decode_chain_ref's list: the scratch buffers hold the last layer's values"""
    last = res[-1]
    return dict(x=last["x2"], qkv=last["qkv"], att=last["att"], g=last["g"], ssq_a=last["ssq_a"], ssq_b=last["ssq_b"],
                kc=[r["kc"] for r in res], vc=[r["vc"] for r in res])


# ---------------------------------------------------------------------------------------------------------------- fixtures
def _tok(x):
    """[B, heads, T, d] -> the cache layout [B, T, heads * d]"""
    B, Hh, Tn, d = x.shape
    return x.permute(0, 2, 1, 3).reshape(B, Tn, Hh * d).contiguous()


def interleave(wg, wu):
    """gate and up rows [F, H] in 16-row [gate | up] groups -> [2F, H]"""
    F_ = wg.shape[0]
    return torch.stack([wg.view(F_ // 16, 16, -1), wu.view(F_ // 16, 16, -1)], 1).reshape(2 * F_, -1)


def gamma(n, seed):
    """norm weights away from 1, so that the fold matters"""
    return (1.0 + 0.5 * T.rand((n,), seed)).clamp(0.25, 2.5)


def dense_weights(hidden, ffn, seed):
    """bf16 Gaussians scaled by K ** -0.5, gamma folded into q|k|v and gate|up -> (wqkv, wo, wgu, wd)"""
    g1, g2 = gamma(hidden, seed + 5), gamma(hidden, seed + 6)
    wqkv = (T.rand((3 * hidden, hidden), seed, hidden ** -0.5) * g1[None, :]).to(BF16)
    wo = T.rand((hidden, hidden), seed + 1, hidden ** -0.5).to(BF16)
    wgu = (interleave(T.rand((ffn, hidden), seed + 2, hidden ** -0.5), T.rand((ffn, hidden), seed + 3, hidden ** -0.5)) * g2[None, :]).to(BF16)
    wd = T.rand((hidden, ffn), seed + 4, ffn ** -0.5).to(BF16)
    return wqkv, wo, wgu, wd


def onehot_fixture(hidden, heads, ffn, nks, seed):
    """One layer whose answer is known: x = e_m and stats0 = (0, 1) with wqkv[:, m] = qkv_raw[m] make stage 0 hand on qkv_raw bit
    for bit; qkv_raw, the caches and the table are attn_edge_ref.rope_case's with chain_choice, so att is the chosen V row; wo is a
    signed permutation and wd = 0, so the final x is r16(+-att[perm] + x), exactly (asserted). wgu is dense."""
    M = len(nks)
    assert hidden == heads * D and M <= 8
    c, qkv_raw, k0, v0, cs = A.rope_case(M, heads, TMAX, list(nks), seed, BF16, choice=A.chain_choice(M, heads, nks, shift=seed))
    x0 = torch.zeros((M, hidden), dtype=BF16)
    x0[torch.arange(M), torch.arange(M)] = 1.0
    stats0 = torch.tensor([[0.0, 1.0]] * M, dtype=F32)
    wqkv = torch.zeros((3 * hidden, hidden), dtype=BF16)
    wqkv[:, :M] = qkv_raw.reshape(M, 3 * hidden).T
    gen = torch.Generator(device="cpu").manual_seed(seed + 7)
    perm = torch.randperm(hidden, generator=gen)
    sign = (torch.randint(0, 2, (hidden,), generator=gen) * 2 - 1).double()
    wo = torch.zeros((hidden, hidden), dtype=BF16)
    wo[torch.arange(hidden), perm] = sign.to(BF16)
    _, _, wgu, _ = dense_weights(hidden, ffn, seed + 20)
    wd = torch.zeros((hidden, ffn), dtype=BF16)
    att = c.v_choice()[:, :, 0].reshape(M, hidden)
    x_expect = G.to16(sign[None, :] * att.double()[:, perm] + x0.double(), BF16, exact=True)
    return dict(geom=(hidden, heads, ffn), nks=tuple(nks), case=c, qkv_raw=qkv_raw.reshape(M, 3 * hidden), x=x0, stats0=stats0, cos_sin=cs,
                layers=[(wqkv, wo, wgu, wd, _tok(k0), _tok(v0))], att=att, x_expect=x_expect, k_rot64=c.k_rot64.reshape(M, hidden))


def dense_fixture(hidden, heads, ffn, nks, n_layers, seed):
    """Gaussian operands: x rows at different scales, stats0 from the float64 rms of x, every layer with weights and caches of its
    own, cache rows from nk_rows[b] - 1 on NaN."""
    M = len(nks)
    x = (T.rand((M, hidden), seed) * (0.5 + 0.3 * torch.arange(M))[:, None]).to(BF16)
    rstd = 1.0 / torch.sqrt((x.double() ** 2).mean(1) + EPS)
    stats0 = torch.stack([torch.zeros(M, dtype=F64), rstd], 1).float()
    layers = []
    for li in range(n_layers):
        sd = seed + 100 * (li + 1)
        kc, vc = T.rand((M, TMAX, hidden), sd + 10).to(BF16), T.rand((M, TMAX, hidden), sd + 11).to(BF16)
        for b, n in enumerate(nks):
            kc[b, n - 1:], vc[b, n - 1:] = NAN, NAN
        layers.append(dense_weights(hidden, ffn, sd) + (kc, vc))
    return dict(geom=(hidden, heads, ffn), nks=tuple(nks), x=x, stats0=stats0, cos_sin=A.cos_sin_table(TMAX, D), layers=layers)


def with_wd_zero(layers, li):
    """the same table with layer li's down_proj weights zero: its final x is then x after o_proj"""
    out = list(layers)
    w = out[li]
    out[li] = w[:3] + (torch.zeros_like(w[3]),) + w[4:]
    return out


# ------------------------------------------------------------------------------------------------------------------ checks
# Every check returns {name: ratio}: |got - ref| over its bound, 0 / inf for an equality. The caller asserts ratio <= 1.
def _eq(a, b):
    """bitwise equality of two tensors of one 16- or 32-bit type, NaN included"""
    a, b = a.contiguous(), b.contiguous()
    it = torch.int16 if a.element_size() == 2 else torch.int32
    return 0.0 if a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.view(it), b.view(it)) else T.INF


def dev16(t):
    """a launch result as the 16-bit tensor it is (the restatement's float64 stand-ins hold bf16 values)"""
    if t.dtype == BF16:
        return t
    out = t.float().to(BF16)
    out[torch.isnan(out)] = NAN      # (one NaN pattern, the fixtures': a wide conversion does not keep it)
    return out


def same_launch(a, b, names=("x", "qkv", "att", "g", "ssq_a", "ssq_b", "kc", "vc")):
    """two launch results bit for bit"""
    out = {}
    for n in names:
        pa, pb = (a[n], b[n]) if isinstance(a[n], list) else ([a[n]], [b[n]])
        out["same " + n] = max([_eq(s, t) for s, t in zip(pa, pb)] + [0.0 if len(pa) == len(pb) else T.INF])
    return out


def check_product(got, ref, ev32):
    return T.ratio(got, ref, T.bound(ref, ev32, BF16))


def check_ssq(got, x16, M):
    """got [H / 16, >= M] fp32 against the float64 group sums of the stored x16 [M, H]"""
    terms = (x16.double() ** 2).view(M, -1, 16)
    ref = terms.sum(-1)
    bnd = T.sum_bound(terms, T.seq_sum32(terms, dim=-1), ref, dim=-1)
    return T.ratio(got[:, :M].T, ref, bnd)


def check_swiglu(got, x1, wgu, ssq_a, M, H):
    """g against silu(gate) * up on the device's own x and ssq_a: the fp32 evaluation's error (train_edge_ref.bound without a
    storage ulp) plus the exponential form's (gemm_edge_ref.bound) bound the fp32 value; the stored bf16 is one rounding of an
    admissible value (gemm_edge_ref.interval16). -> (ratio of |got - ref| to that bound plus half a storage ulp, inside the interval)"""
    if not (bool(torch.isfinite(x1.double()).all()) and bool(torch.isfinite(ssq_a.double()[:, :M]).all())):
        return T.INF, False      # (the stage's own inputs are not numbers: nothing to restate)
    gate, up = gate_up_pre(x1, wgu, rstd_of_ssq(ssq_a, M, H))
    ref = gate *torch.sigmoid(gate) * up
    ev32 = stage_gate_up(x1, wgu, rstd_of_ssq(ssq_a, M, H, dt=F32), rnd=False, dt=F32)
    b = T.bound(ref, ev32, F32) + G.bound(gate, G.ACT_SILU, up)
    lo, hi = G.interval16(ref, b, BF16)
    g = got.double()
    inside = bool(((g >= lo.double()) & (g <= hi.double())).all())
    return T.ratio(got, ref, b + T.half_ulp(ref, BF16)), inside


def check_k_row(kc_after, k_rot64, nks):
    """the appended K rows [M, H] in storage ulps from the float64 rotation"""
    worst = 0.0
    for b, n in enumerate(nks):
        d = (kc_after[b, n - 1].double() - k_rot64[b]).abs() / A.ulp(k_rot64[b], BF16)
        worst = max(worst, float(torch.nan_to_num(d, nan=T.INF).max()))
    return worst


def check_other_rows(after, before, nks):
    """every cache row but the appended one keeps its bits"""
    worst = 0.0
    for b, n in enumerate(nks):
        keep = torch.arange(before.shape[1]) != n - 1
        worst = max(worst, _eq(dev16(after[b][keep]), before[b][keep]))
    return worst


def check_onehot(fx, got):
    """the one-layer launch on onehot_fixture"""
    (hidden, heads, ffn), nks = fx["geom"], fx["nks"]
    M = len(nks)
    wqkv, wo, wgu, wd, k0, v0 = fx["layers"][0]
    kc, vc = got["kc"][0], got["vc"][0]
    out = {"qkv == qkv_raw": _eq(dev16(got["qkv"]), fx["qkv_raw"]),
           "att == chosen V row": _eq(dev16(got["att"]), fx["att"]),
           "appended V row": max(_eq(dev16(vc[b, n - 1]), fx["qkv_raw"][b, 2 * hidden:]) for b, n in enumerate(nks)),
           "appended K row (ulps)": check_k_row(kc, fx["k_rot64"], nks),
           "other K rows": check_other_rows(kc, k0, nks), "other V rows": check_other_rows(vc, v0, nks),
           "x == r16(+-att[perm] + x0)": _eq(dev16(got["x"]), fx["x_expect"]),
           "ssq_a": check_ssq(got["ssq_a"], fx["x_expect"], M), "ssq_b": check_ssq(got["ssq_b"], fx["x_expect"], M)}
    out["g"], inside = check_swiglu(got["g"], got["x"], wgu, got["ssq_a"], M, hidden)
    out["g inside its interval"] = 0.0 if inside else T.INF
    return out


def check_layer(fx, li, prev, got0, got1):
    """Layer li of dense_fixture, teacher-forced: got0 is the (li + 1)-layer launch with layer li's wd = 0 (its final x is x after
    o_proj), got1 the same launch with the real wd, prev the li-layer launch (None for li = 0): its final x and ssq_b are what layer
    li starts from. Every stage against its restatement on the DEVICE's inputs to that stage."""
    (hidden, heads, ffn), nks = fx["geom"], fx["nks"]
    M = len(nks)
    wqkv, wo, wgu, wd, k0, v0 = fx["layers"][li]
    x_in = fx["x"] if li == 0 else dev16(prev["x"])
    rstd = (lambda dt: fx["stats0"][:, 1].to(dt)) if li == 0 else (lambda dt: rstd_of_ssq(prev["ssq_b"], M, hidden, dt=dt))
    out = {"stages 0-3 " + k: v for k, v in same_launch(got0, got1, ("qkv", "att", "g", "ssq_a", "kc", "vc")).items()}
    out["qkv"] = check_product(got1["qkv"], stage_qkv(x_in, wqkv, rstd(F64), rnd=False), stage_qkv(x_in, wqkv, rstd(F32), rnd=False, dt=F32))
    kc, vc = got1["kc"][li], got1["vc"][li]
    qkv = dev16(got1["qkv"])
    k_row = torch.stack([kc[b, n - 1] for b, n in enumerate(nks)])
    a = stage_attention(qkv, k0, v0, fx["cos_sin"], nks, heads, rnd=True, k_row=k_row)
    a64 = stage_attention(qkv, k0, v0, fx["cos_sin"], nks, heads, rnd=False)
    out["appended K row (ulps)"] = check_k_row(kc, a64["k_rot"], nks)
    out["appended V row"] = max(_eq(dev16(vc[b, n - 1]), qkv[b, 2 * hidden:]) for b, n in enumerate(nks))
    out["other K rows"], out["other V rows"] = check_other_rows(kc, k0, nks), check_other_rows(vc, v0, nks)
    # (q and k rotated and rounded as the kernel stores them, the device's own appended K row, softmax and P.V unrounded)
    out["att"] = T.ratio(got1["att"], a["att_unrounded"], A.bound(a["att_unrounded"], a["vmax"], BF16, A.U32))
    att, x1 = dev16(got1["att"]), dev16(got0["x"])
    out["x after o_proj"] = check_product(x1, stage_oproj(att, wo, x_in, rnd=False)[0], stage_oproj(att, wo, x_in, rnd=False, dt=F32)[0])
    out["ssq_a"] = check_ssq(got1["ssq_a"], x1, M)
    out["ssq_b (wd = 0)"] = check_ssq(got0["ssq_b"], x1, M)
    out["g"], inside = check_swiglu(got1["g"], x1, wgu, got1["ssq_a"], M, hidden)
    out["g inside its interval"] = 0.0 if inside else T.INF
    g = dev16(got1["g"])
    out["x after down_proj"] = check_product(got1["x"], stage_down(g, wd, x1, rnd=False)[0], stage_down(g, wd, x1, rnd=False, dt=F32)[0])
    out["ssq_b"] = check_ssq(got1["ssq_b"], dev16(got1["x"]), M)
    if prev is not None:     # the layers below appended what the shorter launch appended
        for l2 in range(li):
            out[f"layer {l2} cache rows as the shorter launch"] = max(_eq(dev16(got1["kc"][l2]), dev16(prev["kc"][l2])), _eq(dev16(got1["vc"][l2]), dev16(prev["vc"][l2])),
                                                                       _eq(dev16(got0["kc"][l2]), dev16(prev["kc"][l2])), _eq(dev16(got0["vc"][l2]), dev16(prev["vc"][l2])))
    return out


def check_prefix(fx, launch):
    """launch(layers) -> the result of one launch over those layers. Layer by layer: the (li + 1)-layer launch with and without
    layer li's down_proj, checked against the li-layer launch (check_layer) -> {"L<li> <name>": ratio}"""
    out, prev = {}, None
    for li in range(len(fx["layers"])):
        got0, got1 = launch(with_wd_zero(fx["layers"], li)[:li + 1]), launch(fx["layers"][:li + 1])
        out.update({f"L{li} {k}": v for k, v in check_layer(fx, li, prev, got0, got1).items()})
        prev = got1
    return out


def restatement_launch(fx, **wrong):
    """the launch(layers) of check_prefix / check_onehot answered by this restatement (with a mistake switched on)"""
    return lambda layers: as_launch(decode_chain_ref(layers, fx["x"], fx["stats0"], fx["cos_sin"], fx["nks"], fx["geom"][1], **wrong))
