"""Serving LoRA adapters unmerged on the NF4 base, host side (no GPU): the two entry points' declarations (their host-side refusals:
tests/test_quant_contract_cpu.py), LisaMI355's option refusals, the adapter layout quant.lora_pack builds, the CPU restatement (tests/lora_serve_ref.py) by hand, and
what the GPU comparisons' tolerance can and cannot pass."""
import ctypes
import os
import re
import sys

import pytest
import torch

import haff

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/nf4_ref.py, tests/lora_serve_ref.py
import lora_serve_ref as LR   # noqa: E402
import nf4_ref as R   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("haff_nf4_dequant_lora_f16", "haff_gemm_nf4_lora_f16")


def test_declarations_equal_the_ctypes_prototypes():
    from haff import lib as hlib
    text = open(os.path.join(ROOT, "include", "haff_hip.h")).read()
    ctype = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float}
    for name in NAMES:
        m = re.search(r"^int " + name + r"\((.*?)\);", text, flags=re.M | re.S)
        assert m, name
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        want = [ctypes.c_void_p if "*" in p else ctype[p.replace("const ", "").split()[0]] for p in params]
        assert hlib._PROTOS[name] == want, (name, params)
        assert name in haff.EXPORTED_SYMBOLS
    # each is its parent's argument list with the adapters' arguments in front of the stream
    assert hlib._PROTOS[NAMES[0]][:7] + hlib._PROTOS[NAMES[0]][-1:] == hlib._PROTOS["haff_nf4_dequant_f16"]
    assert hlib._PROTOS[NAMES[1]][:16] + hlib._PROTOS[NAMES[1]][-1:] == hlib._PROTOS["haff_gemm_nf4_f16"]


def _state(cfg, modules, r=8):
    H, F = cfg.llm.hidden, cfg.llm.ffn
    dims = {"q_proj": (H, H), "k_proj": (H, H), "v_proj": (H, H), "o_proj": (H, H), "gate_proj": (H, F), "up_proj": (H, F),
            "down_proj": (F, H)}
    out = {}
    for m in modules:
        fin, fout = dims[m.rsplit(".", 1)[1]]
        out[m + ".lora_A"], out[m + ".lora_B"] = torch.zeros(r, fin), torch.zeros(fout, r)
    return out


def test_option_refusals_name_the_offender(tmp_path):
    from haff import config as hcfg
    from haff.lisa import LisaMI355
    cfg = hcfg.tiny()
    q0 = "model.layers.0.self_attn.q_proj"
    new = lambda st, **kw: LisaMI355(cfg, {}, dtype=torch.float16, load_in_4bit=True, lora_state=st, **kw)   # noqa: E731
    with pytest.raises(ValueError, match="16-bit bases are served merged"):
        LisaMI355(cfg, {}, dtype=torch.float16, lora_state=_state(cfg, [q0]))
    with pytest.raises(ValueError, match="16-bit bases are served merged"):
        LisaMI355(cfg, {}, dtype=torch.bfloat16, lora_state=_state(cfg, [q0]))
    with pytest.raises(ValueError, match=r"lm_head is not one of the Llama projections"):
        new({"lm_head.lora_A": torch.zeros(8, cfg.llm.hidden), "lm_head.lora_B": torch.zeros(cfg.llm.vocab, 8)})
    with pytest.raises(ValueError, match=r"model\.mm_projector is not one of"):
        new({"model.mm_projector.lora_A": torch.zeros(8, 8), "model.mm_projector.lora_B": torch.zeros(8, 8)})
    with pytest.raises(ValueError, match=rf"model\.layers\.{cfg.llm.layers}\.mlp\.up_proj is not one of"):
        new(_state(cfg, [f"model.layers.{cfg.llm.layers}.mlp.up_proj"]))
    with pytest.raises(ValueError, match=r"layers\.0\.mlp\.down_proj has rank 16"):
        new(_state(cfg, ["model.layers.0.mlp.down_proj"], r=16))
    st = _state(cfg, [q0])
    st[q0 + ".lora_B"] = torch.zeros(cfg.llm.hidden + 16, 8)
    with pytest.raises(ValueError, match=r"q_proj: lora_A .* do not fit"):
        new(st)
    st = _state(cfg, ["model.layers.0.mlp.gate_proj"])
    st["model.layers.0.mlp.gate_proj.lora_A"] = torch.zeros(8, cfg.llm.ffn)       # in_features of down_proj, not of gate_proj
    with pytest.raises(ValueError, match=r"gate_proj: lora_A .* do not fit"):
        new(st)
    st = _state(cfg, [q0])
    del st[q0 + ".lora_B"]
    with pytest.raises(ValueError, match=r"q_proj has only one of"):
        new(st)
    st = _state(cfg, [q0], r=4)
    st.update(_state(cfg, ["model.layers.0.self_attn.v_proj"], r=8))
    with pytest.raises(ValueError, match=r"has rank"):
        new(st)
    # checkpoints: a 16-bit fine-tune's is refused by name, and so is any without load_in_4bit
    for fmt in (None, "bf16"):
        p = tmp_path / f"latest_{fmt}.pt"
        torch.save({"params": _state(cfg, [q0]), "base_format": fmt}, p)
        with pytest.raises(ValueError, match=r"latest_.*base_format=.*merge_lora"):
            LisaMI355.read_lora_checkpoint(str(p))
    p = tmp_path / "latest_nf4.pt"
    torch.save({"params": _state(cfg, [q0]), "base_format": "nf4"}, p)
    assert set(LisaMI355.read_lora_checkpoint(str(p))) == {q0 + ".lora_A", q0 + ".lora_B"}
    with pytest.raises(ValueError, match="load_in_4bit=True"):
        LisaMI355.read_lora_checkpoint(str(p), load_in_4bit=False)
    torch.save(_state(cfg, [q0]), tmp_path / "bare.pt")
    with pytest.raises(ValueError, match="no 'params' entry"):
        LisaMI355.read_lora_checkpoint(str(tmp_path / "bare.pt"))
    # the refusals that existed before keep their precedence
    with pytest.raises(ValueError, match="float16"):
        LisaMI355(cfg, {}, dtype=torch.bfloat16, load_in_4bit=True, lora_state=_state(cfg, [q0]))


def test_lora_pack_follows_the_quantisers_row_order():
    from haff import quant
    g = torch.Generator().manual_seed(2)
    H, F, K = 32, 48, 64
    rnd = lambda *s: torch.rand(s, generator=g) - 0.5   # noqa: E731
    aq, bq, av, bv = rnd(8, K), rnd(H, 8), rnd(4, K), rnd(H, 4)
    L = quant.lora_pack([((aq, bq), H, None), (None, H, None), ((av, bv), H, None)], K, H, 2.0, "cpu")
    assert (L.nseg, L.seg_rows, L.scale) == (3, H, 2.0) and L.a_cat.shape == (24, K) and L.b.shape == (3 * H, 8)
    assert L.a_cat.dtype == torch.float16 and L.b.dtype == torch.float16
    assert torch.equal(L.a_cat[:8], aq.half()) and (L.a_cat[8:16] == 0).all()
    assert torch.equal(L.a_cat[16:20], av.half()) and (L.a_cat[20:] == 0).all()          # rank 4: zero-padded
    assert torch.equal(L.b[:H], bq.half()) and (L.b[H:2 * H] == 0).all()
    assert torch.equal(L.b[2 * H:, :4], bv.half()) and (L.b[2 * H:, 4:] == 0).all()
    # what the layout means: the update of stored row n is B[n] . A_cat[8 seg(n) ..]
    upd = LR.update(torch.eye(K).half() @ L.a_cat.T.float().half(), L.b, 3, H, 1.0)       # t of the unit rows: a_cat^T
    want = torch.cat([bq.half().double() @ aq.half().double(), torch.zeros(H, K).double(), bv.half().double() @ av.half().double()])
    assert torch.allclose(upd.T, want, atol=1e-12)
    # gate | up through quant.swiglu_rows: stored row 32 i + j is gate row 16 i + j, 32 i + 16 + j up row 16 i + j
    ag, bg, au, bu = rnd(8, K), rnd(F, 8), rnd(8, K), rnd(F, 8)
    gr, ur = quant.swiglu_rows(F)
    L = quant.lora_pack([((ag, bg), F, gr), ((au, bu), F, ur)], K, 16, 2.0, "cpu")
    assert (L.nseg, L.seg_rows) == (2, 16)
    seg = LR.seg_of(2 * F, 2, 16)
    assert torch.equal(L.b[seg == 0], bg.half()) and torch.equal(L.b[seg == 1], bu.half())
    assert torch.equal(L.b[32:48], bg.half()[16:32]) and torch.equal(L.b[48:64], bu.half()[16:32])
    assert quant.lora_pack([(None, H, None)], K, 16, 2.0, "cpu") is None


def test_restatement_by_hand():
    c = LR.make_case(3, 64, 128, 2, 16, 0)
    zero = torch.zeros_like(c["b"])
    # without adapters: nf4_ref.dequant's bits and nf4_ref.product's values
    assert torch.equal(LR.dequant_lora(c["packed"], c["absmax"], c["a_cat"], zero, 2, 16, 2.0).view(torch.int16),
                       c["wdeq"].view(torch.int16))
    assert torch.equal(LR.product_lora(c["x"], c["packed"], c["absmax"], c["t"], zero, 2, 16, 2.0), R.product(c["x"], c["packed"], c["absmax"]))
    # one element by hand, in the stated order: row 21 is in segment 1 (rows 16..31)
    n, k = 21, 77
    code = int(c["packed"][n, k // 2] & 15)
    d = R.NF4[code] * c["absmax"][n, k // 64]
    u = torch.tensor(0.0)
    for j in range(8):
        u = u + c["b"][n, j].float() * c["a_cat"][8 + j, k].float()
    want = (d + torch.tensor(2.0) * u).half()
    got = LR.dequant_lora(c["packed"], c["absmax"], c["a_cat"], c["b"], 2, 16, 2.0)
    assert got[n, k].item() == want.item() and got[n, k].item() != c["wdeq"][n, k].item()
    m = 2
    y = (c["x"][m].double() * c["wdeq"][n].double()).sum() + 2.0 * (c["t"][m, 8:16].double() * c["b"][n].double()).sum()
    assert abs(LR.product_lora(c["x"], c["packed"], c["absmax"], c["t"], c["b"], 2, 16, 2.0)[m, n].item() - y.item()) < 1e-12
    # the dequantised form and the product form are the same function up to the f16 rounding of the weights and of t
    eff = LR.dequant_lora(c["packed"], c["absmax"], c["a_cat"], c["b"], 2, 16, 2.0).double()
    y2 = LR.product_lora(c["x"], c["packed"], c["absmax"], c["t"], c["b"], 2, 16, 2.0)
    assert ((c["x"].double() @ eff.T - y2).abs() <= 2e-3 * R.magnitude(c["x"], eff)).all()


SHAPES = [(1, 64, 64), (17, 96, 448), (64, 512, 4096), (33, 256, 13824)]


@pytest.mark.parametrize("out_dtype", [torch.float16, torch.float32])
@pytest.mark.parametrize("M,N,K", SHAPES)
def test_adapters_contribution_is_far_above_the_tolerance(M, N, K, out_dtype):
    """The input condition of the product tests: with init_lora(init_b_zero=False)'s distributions the update is at least 15x the
    tolerance in L2 norm and exceeds it on more than 95 % of the outputs, so a kernel that drops or garbles it cannot pass."""
    c = LR.make_case(M, N, K, 2, 16, 100 + M)
    upd = LR.update(c["t"], c["b"], 2, 16, 2.0)
    ref = LR.product_lora(c["x"], c["packed"], c["absmax"], c["t"], c["b"], 2, 16, 2.0)
    tol = LR.tol(c["x"], c["wdeq"], None, out_dtype, c["t"], c["b"], 2, 16, 2.0, ref)
    ratio = (upd.norm() / tol.norm()).item()
    share = (upd.abs() > tol).double().mean().item()
    print(f"({M},{N},{K}) {out_dtype}: |update| / |tol| = {ratio:.1f}, above tolerance on {100 * share:.1f} %")
    assert ratio >= 15 and share > 0.95


@pytest.mark.parametrize("out_dtype", [torch.float32, torch.float16])
def test_tolerance_rejects_kernel_mistakes(out_dtype):
    """On the reference alone: each mistake the epilogue of haff_gemm_nf4_lora_f16 can make lies outside the tolerance on at least
    1 % of the outputs (the exact result, rounded to the output format, lies inside everywhere)."""
    M, N, K, nseg, sr, s = 33, 96, 448, 3, 32, 2.0
    c = LR.make_case(M, N, K, nseg, sr, 7)
    x, p, a, t, b = c["x"], c["packed"], c["absmax"], c["t"], c["b"]
    ref = LR.product_lora(x, p, a, t, b, nseg, sr, s)
    tol = LR.tol(x, c["wdeq"], None, out_dtype, t, b, nseg, sr, s, ref)
    assert ((ref.to(out_dtype).double() - ref).abs() <= tol).all()
    t_nb = t.view(M, nseg, 8).roll(1, dims=1).reshape(M, 8 * nseg)          # segment i reads segment i - 1's rank values
    mutations = {
        "the neighbouring segment's A rows": LR.product_lora(x, p, a, t_nb, b, nseg, sr, s),
        "the scale dropped": LR.product_lora(x, p, a, t, b, nseg, sr, 1.0),
        "t of another activation row": LR.product_lora(x, p, a, t.roll(1, dims=0), b, nseg, sr, s),
        "B shifted by one row": LR.product_lora(x, p, a, t, b.roll(1, dims=0), nseg, sr, s),
        "the update left out": R.product(x, p, a),
    }
    for name, mut in mutations.items():
        share = ((mut - ref).abs() > tol).double().mean().item()
        assert share >= 0.01, (name, share)
