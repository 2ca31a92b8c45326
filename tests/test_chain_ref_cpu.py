"""tests/chain_ref.py on its own, without a GPU:
  * with round_handoffs=False the restatement of the chained decode step is a textbook Llama decoder stack in float64 (gamma not
    folded, gate and up apart, rotate-half RoPE, attention recomputed over the whole token history without a cache) to 1e-12;
  * with the roundings on, the K row it appends is attn_edge_ref.rope rounded once;
  * the per-stage functions composed by hand are decode_chain_ref bit for bit;
  * every fixture of tests/test_chain_edge_kernels_gpu.py builds (the builders assert their own margins and exactness), the
    attention stages have 2 .. 32 workgroups on both sides of the 8 counter shards, every key of chain_choice is some row's answer;
  * the restatement passes the GPU module's checks, and with any one of MISTAKES switched on at least one of them fails by 10x."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_edge_ref as A   # noqa: E402
import chain_ref as C   # noqa: E402
import gemm_edge_ref as G   # noqa: E402
import train_edge_ref as T   # noqa: E402

F64, BF16 = torch.float64, torch.bfloat16


# --------------------------------------------------------------------------------------------------------- textbook layer
def _rotate_half(x):
    return torch.cat([-x[..., x.shape[-1] // 2:], x[..., :x.shape[-1] // 2]], -1)


def _rms(x, w, eps):
    return x / torch.sqrt((x * x).mean(-1, keepdim=True) + eps) * w


def _textbook_layer(h, p, cs, heads, eps, scale):
    """LlamaDecoderLayer on the whole history h [Tn, H] (positions 0 .. Tn - 1), causal -> (h out, rotated K, V [Tn, H])"""
    Tn, H = h.shape
    d = H // heads
    a = _rms(h, p["n1"], eps)
    q, k, v = ((a @ p[n].T).view(Tn, heads, d) for n in ("wq", "wk", "wv"))
    cos, sin = (torch.cat([t, t], -1)[:, None, :] for t in (cs[:Tn, :d // 2], cs[:Tn, d // 2:]))
    q, k = q * cos + _rotate_half(q) * sin, k * cos + _rotate_half(k) * sin
    s = torch.einsum("ihd,jhd->hij", q, k) * scale      # (1 / sqrt(d) as the fp32 argument carries it, like eps)
    s = s.masked_fill(torch.arange(Tn)[None, :] > torch.arange(Tn)[:, None], -float("inf"))
    o = torch.einsum("hij,jhd->ihd", torch.softmax(s, -1), v).reshape(Tn, H)
    h = h + o @ p["wo"].T
    m = _rms(h, p["n2"], eps)
    gate = m @ p["wg"].T
    return h + (gate * torch.sigmoid(gate) * (m @ p["wu"].T)) @ p["wd"].T, k.reshape(Tn, H), v.reshape(Tn, H)


def test_unrounded_restatement_is_a_textbook_llama_layer():
    hidden, heads, ffn, n_layers, nks = 256, 2, 512, 3, (7, 1, 12, 2, 9)
    M, tmax, eps = len(nks), 16, C.EPS
    cs = A.cos_sin_table(tmax, C.D).double()
    r = lambda shape, seed, s=1.0: T.rand(shape, seed, s).double()   # noqa: E731
    params = [dict(wq=r((hidden, hidden), 10 * l + 1, hidden ** -0.5), wk=r((hidden, hidden), 10 * l + 2, hidden ** -0.5), wv=r((hidden, hidden), 10 * l + 3, hidden ** -0.5),
                   wo=r((hidden, hidden), 10 * l + 4, hidden ** -0.5), wg=r((ffn, hidden), 10 * l + 5, hidden ** -0.5), wu=r((ffn, hidden), 10 * l + 6, hidden ** -0.5),
                   wd=r((hidden, ffn), 10 * l + 7, ffn ** -0.5), n1=C.gamma(hidden, 10 * l + 8).double(), n2=C.gamma(hidden, 10 * l + 9).double()) for l in range(n_layers)]
    hist = [r((n, hidden), 50 + b, 0.5 + 0.3 * b) for b, n in enumerate(nks)]      # every row's token history, the new token last
    # the textbook stack on every history; its K / V of the earlier positions are what the caches hold
    want = [[] for _ in range(n_layers)]
    kcs = [torch.full((M, tmax, hidden), C.NAN, dtype=F64) for _ in range(n_layers)]
    vcs = [torch.full((M, tmax, hidden), C.NAN, dtype=F64) for _ in range(n_layers)]
    for b, n in enumerate(nks):
        h = hist[b]
        for l in range(n_layers):
            h, k, v = _textbook_layer(h, params[l], cs, heads, eps, T.f32(C.SCALE))
            want[l].append(h[-1])
            kcs[l][b, :n - 1], vcs[l][b, :n - 1] = k[:-1], v[:-1]
    layers = [(torch.cat([p["wq"], p["wk"], p["wv"]]) * p["n1"][None, :], p["wo"], C.interleave(p["wg"], p["wu"]) * p["n2"][None, :], p["wd"], kcs[l], vcs[l])
              for l, p in enumerate(params)]
    x = torch.stack([h[-1] for h in hist])
    stats0 = torch.stack([torch.zeros(M, dtype=F64), 1.0 / torch.sqrt((x * x).mean(1) + eps)], 1)
    res = C.decode_chain_ref(layers, x, stats0, cs, nks, heads, eps, round_handoffs=False)
    for l in range(n_layers):
        ref = torch.stack(want[l])
        err = float((res[l]["x2"] - ref).abs().max() / ref.abs().max())
        assert err <= 1e-12, (l, err)
        assert bool(torch.isnan(res[l]["kc"][0, nks[0]:]).all()) and not bool(torch.isnan(res[l]["kc"][0, :nks[0]]).any())


# --------------------------------------------------------------------------------------------------- the restatement itself
def _dense(n_layers=2, geom=C.GEOMS[1], nks=C.NK_GROUPS[4], seed=3):
    return C.dense_fixture(*geom, nks, n_layers, seed)


def test_appended_k_row_is_rope_rounded_once():
    fx = _dense(1)
    hidden, heads, _ = fx["geom"]
    M = len(fx["nks"])
    res = C.decode_chain_ref(fx["layers"], fx["x"], fx["stats0"], fx["cos_sin"], fx["nks"], heads)[0]
    pos = torch.tensor([n - 1 for n in fx["nks"]])
    k = res["qkv"][:, hidden:2 * hidden].reshape(M, heads, C.D)
    want = G.to16(A.rope(k, pos[:, None], fx["cos_sin"]), BF16).reshape(M, hidden)
    for b, n in enumerate(fx["nks"]):
        assert torch.equal(res["kc"][b, n - 1].to(BF16), want[b])
        assert torch.equal(res["vc"][b, n - 1], res["qkv"][b, 2 * hidden:])
    assert C.check_k_row(res["kc"], A.rope(k, pos[:, None], fx["cos_sin"]).reshape(M, hidden), fx["nks"]) <= 0.5


def test_stage_functions_compose_to_the_whole_step():
    fx = _dense(2)
    hidden, heads, _ = fx["geom"]
    M, nks = len(fx["nks"]), fx["nks"]
    res = C.decode_chain_ref(fx["layers"], fx["x"], fx["stats0"], fx["cos_sin"], nks, heads)
    x, rstd = fx["x"].double(), fx["stats0"].double()[:, 1]
    for li, (wqkv, wo, wgu, wd, kc, vc) in enumerate(fx["layers"]):
        qkv = C.stage_qkv(x, wqkv, rstd)
        a = C.stage_attention(qkv, kc, vc, fx["cos_sin"], nks, heads)
        x1, ssq_a = C.stage_oproj(a["att"], wo, x)
        g = C.stage_gate_up(x1, wgu, C.rstd_of_ssq(ssq_a, M, hidden))
        x2, ssq_b = C.stage_down(g, wd, x1)
        mine = dict(qkv=qkv, att=a["att"], q_rot=a["q_rot"], k_rot=a["k_rot"], kc=a["kc"], vc=a["vc"], x1=x1, ssq_a=ssq_a, g=g, x2=x2, ssq_b=ssq_b)
        for name, t in mine.items():
            assert C._eq(t, res[li][name]) == 0.0, (li, name)
        x, rstd = x2, C.rstd_of_ssq(ssq_b, M, hidden)
    # the hand-offs hold bf16 values, the unrounded step does not
    assert G.is16(res[1]["x2"], BF16) and G.is16(res[1]["g"], BF16) and G.is16(res[1]["q_rot"], BF16)
    assert not G.is16(C.decode_chain_ref(fx["layers"], fx["x"], fx["stats0"], fx["cos_sin"], nks, heads, round_handoffs=False)[1]["x2"], BF16)


# ------------------------------------------------------------------------------------------------------------- fixtures
def test_every_fixture_builds_and_the_cases_cover_the_edges():
    assert C.attn_workgroups() == [2, 4, 6, 8, 10, 12, 16, 20, 32]
    assert {len(nks) for _, nks in C.dense_cases()} == set(range(1, 9))
    kinds = set()
    for i, ((hidden, heads, ffn), nks) in enumerate(C.onehot_cases()):
        fx = C.onehot_fixture(hidden, heads, ffn, nks, 40 + i)      # rope_case asserts the margin, to16(exact=True) the exact x
        assert A.assert_margin(fx["case"]) >= A.MARGIN
        ch = fx["case"].choice[..., 0]
        for b, n in enumerate(nks):
            assert bool(torch.isnan(fx["layers"][0][4][b, n - 1:]).all()) and bool(torch.isnan(fx["layers"][0][5][b, n - 1:]).all())
            for h in range(heads):
                key = int(ch[b, h])
                assert 0 <= key < n
                kinds.add("new" if key == n - 1 else "last_cached" if key == n - 2 else key)
        assert G.is16(fx["x_expect"].double(), BF16)
    assert kinds >= {0, "new", "last_cached", 16, 32, 48, 255, 256, 257, 300}, kinds
    for (hidden, heads, ffn), nks in C.dense_cases()[:3]:
        fx = C.dense_fixture(hidden, heads, ffn, nks, 1, 7)
        gate, _ = C.gate_up_pre(fx["x"], fx["layers"][0][2], fx["stats0"][:, 1])
        assert float(gate.abs().max()) <= 16.0


# ----------------------------------------------------------------------------------------------------- checks and mistakes
_FX = {}


def _fixtures():
    if not _FX:
        _FX["onehot"] = [C.onehot_fixture(*C.GEOMS[0], C.NK_GROUPS[2], 41), C.onehot_fixture(*C.GEOMS[0], C.NK_GROUPS[3], 42)]
        _FX["dense"] = _dense(2)
    return _FX


def _all_checks(**wrong):
    out = {}
    for i, fx in enumerate(_fixtures()["onehot"]):
        got = C.restatement_launch(fx, **wrong)(fx["layers"])
        out.update({f"a{i} {k}": v for k, v in C.check_onehot(fx, got).items()})
    fx = _fixtures()["dense"]
    out.update({"c " + k: v for k, v in C.check_prefix(fx, C.restatement_launch(fx, **wrong)).items()})
    return out


def test_the_restatement_passes_the_gpu_modules_checks():
    r = _all_checks()
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, bad


@pytest.mark.parametrize("mistake", C.MISTAKES)
def test_every_mistake_fails_a_check(mistake):
    r = _all_checks(**{mistake: True})
    bad = {k: v for k, v in r.items() if not v <= 10.0}
    print(f"{mistake}: fails {sorted(bad)[:6]}{' ...' if len(bad) > 6 else ''}")
    assert bad, f"{mistake} passes every check"
