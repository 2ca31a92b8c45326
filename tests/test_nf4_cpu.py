"""The NF4 4-bit mode's host side (no GPU): the format's tables, hand cases of the CPU restatement (tests/nf4_ref.py), the product's
tables (haff.quant and the kernel's literals) against it, the module selection, the option refusals, and the three entry points'
declarations (their host-side refusals: tests/test_quant_contract_cpu.py)."""
import ctypes
import os
import re
import sys

import pytest
import torch

import haff

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/nf4_ref.py
import nf4_ref as R   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NF4_BITS = [0xbf800000, 0xbf3239b1, 0xbf066b30, 0xbeca32a0, 0xbe91a24d, 0xbe3d353f, 0xbdba7871, 0x00000000,
            0x3da2faff, 0x3e24cae3, 0x3e7c04dd, 0x3ead033a, 0x3ee1a4b8, 0x3f1007ab, 0x3f3913b3, 0x3f800000]


def _bits(t):
    return [int(v) & 0xffffffff for v in t.contiguous().view(torch.int32).tolist()]


def test_nf4_constants_bit_patterns():
    assert _bits(R.NF4) == NF4_BITS


def test_dynamic_map_construction():
    m = R.dynamic_map()
    assert m.dtype == torch.float32 and m.numel() == 256
    assert torch.equal(m, torch.sort(m).values) and torch.unique(m).numel() == 256
    assert int((m == 0).nonzero()) == 127 and m[-1].item() == 1.0
    # the construction adds +1 but no -1: apart from it the map is symmetric (127 magnitudes each side of 0)
    assert torch.equal(m[:127], -m[128:255].flip(0))
    assert m[0].item() > -1.0 and m[254].item() < 1.0
    assert abs(m[128].item() - 5.5e-7) < 1e-12 and abs(m[254].item() - 0.99296875) < 1e-6


def test_restatement_hand_cases():
    # each code value times absmax maps to itself, and the absmax element to +-1
    a = 3.5
    blk = (R.NF4.repeat(4) * a).half()
    packed, amax, _ = R.quantize(blk.reshape(1, 64), double_quant=False)
    assert amax.item() == a
    codes = torch.stack([packed[0] >> 4, packed[0] & 15], 1).reshape(-1)
    assert torch.equal(codes.long(), torch.arange(16).repeat(4))
    assert torch.equal(R.dequant(packed, amax)[0], blk)
    # an all-zero block dequantises to 0 (codes 7); -0.0 as well
    z = torch.zeros(2, 64, dtype=torch.float16)
    z[1, ::2] = -0.0
    packed, amax, _ = R.quantize(z, double_quant=False)
    assert (packed == 0x77).all() and (amax == 0).all() and (R.dequant(packed, amax) == 0).all()
    # midpoints go to the LOWER code; just above them to the upper one (absmax 1: x = w)
    mids = (R.NF4[:-1] + R.NF4[1:]) * 0.5
    for i in (0, 6, 7, 14):
        x = torch.full((64,), 1.0)
        x[1] = mids[i]
        x[3] = torch.nextafter(mids[i], torch.tensor(2.0))
        q = R._nearest(x, R.NF4)
        assert q[0] == 15 and q[1] == i and q[3] == i + 1


def test_double_quant_restatement():
    g = torch.Generator().manual_seed(0)
    w = (torch.randn(48, 640, generator=g) * 0.02).half()
    p0, a0, off = R.quantize(w, double_quant=False)
    p1, a1, off1 = R.quantize(w, double_quant=True)
    assert torch.equal(p0, p1) and off.item() == off1.item()
    assert abs(off.item() - a0.double().mean().item()) <= 1e-6 * a0.double().mean().item()
    assert not torch.equal(a0, a1) and ((a1 - a0).abs() / a0).max().item() < 2e-2   # the 8-bit map is fine near 0
    assert torch.isfinite(a1).all()


def test_product_restatement_by_hand():
    """nf4_ref.product: NF4[code] * absmax rounded to f16 once, then an exact float64 dot product and the bias."""
    codes = torch.arange(64) % 16
    packed = ((codes[0::2] << 4) | codes[1::2]).to(torch.uint8)[None, :]
    absmax = torch.tensor([[0.1]])
    w = (R.NF4[codes] * torch.tensor(0.1, dtype=torch.float32)).half().double()
    x = torch.linspace(-2, 2, 64).half()
    y = R.product(x[None, :], packed, absmax, torch.tensor([0.25]))
    assert y.dtype == torch.float64 and y.item() == (x.double() * w).sum().item() + 0.25
    assert R.magnitude(x[None, :], w[None, :], torch.tensor([-0.25])).item() == (x.double() * w).abs().sum().item() + 0.25
    # the tolerance: C_ACC of the magnitude, plus one f16 ulp (at 2048: 2) or one fp32 ulp of the reference
    t16 = R.tol(x[None, :], w[None, :], None, torch.float16, torch.tensor([[2048.0]], dtype=torch.float64))
    t32 = R.tol(x[None, :], w[None, :], None, torch.float32, torch.tensor([[2048.0]], dtype=torch.float64))
    base = R.C_ACC * (x.double() * w).abs().sum().item()
    assert abs(t16.item() - (base + 2.0)) < 1e-12 and abs(t32.item() - (base + 2.0 ** -12)) < 1e-12
    assert 1e-5 <= R.C_ACC <= 4e-5


def test_tolerance_rejects_kernel_mistakes_at_7b_shape():
    """The GPU comparisons (tests/test_quant_variants_gpu.py) can fail: at K = 4096, one 16-row activation tile and 16 weight
    tiles, nf4_ref.tol with the f16 output term rejects each of the mistakes a tile kernel makes, in most of the outputs it changes."""
    g = torch.Generator().manual_seed(5)
    M, N, K = 16, 256, 4096
    w = (torch.randn(N, K, generator=g) * 0.02).half()
    x = torch.randn(M, K, generator=g).half()
    bias = torch.randn(N, generator=g) * 0.1
    packed, absmax, _ = R.quantize(w)
    wd = R.dequant(packed, absmax)
    ref = R.product(x, packed, absmax, bias)
    tol = R.tol(x, wd, bias, torch.float16, ref)
    assert ((ref.half().double() - ref).abs() <= tol).all()           # the f16 rounding of the exact result passes
    j = 17
    n = torch.arange(N)
    shifted = 16 * (n // 16) + (n % 16 + 1) % 16
    a_nb = absmax.clone()
    a_nb[:, j] = absmax[:, j + 1]
    m_row = ref.clone()
    m_row[15] = ref[14]
    mutations = {
        "one 64-block dropped": ref - x[:, 64 * j:64 * j + 64].double() @ wd[:, 64 * j:64 * j + 64].double().T,
        "a neighbouring block's absmax": R.product(x, packed, a_nb, bias),
        "weight rows shifted by one in their 16-row tile": R.product(x, packed[shifted], absmax[shifted], bias[shifted]),
        "the last row of the M tile from the row before": m_row,
    }
    for name, mut in mutations.items():
        d = (mut - ref).abs()
        changed = d > 0
        rejected = (d > tol) & changed
        assert rejected.sum() >= 0.8 * changed.sum(), (name, int(rejected.sum()), int(changed.sum()))


def test_product_tables_equal_the_restatement():
    from haff import quant
    assert _bits(quant.nf4_table()) == NF4_BITS
    assert torch.equal(quant.dynamic_map(), R.dynamic_map())
    src = open(os.path.join(ROOT, "2handedafforder_amd", "csrc", "gemm_nf4.hip")).read()

    def lits(name):
        body = re.search(name + r"\[\d+\] = \{(.*?)\};", src, flags=re.S).group(1)
        return torch.tensor([float.fromhex(v[:-1]) if "0x" in v else float(v[:-1])
                             for v in re.findall(r"-?[0-9a-fx.p+\-]+f", body)], dtype=torch.float32)
    assert _bits(lits("kNF4")) == NF4_BITS
    assert torch.equal(lits("kDynMap"), R.dynamic_map())


def test_module_selection():
    from haff import quant
    yes = ["model.layers.0.self_attn.q_proj.weight", "model.layers.31.mlp.down_proj.weight", "model.layers.3.mlp.gate_proj.weight",
           "model.mm_projector.weight", "model.text_hidden_fcs.0.0.weight", "model.text_hidden_fcs.0.2.weight", "lm_head.weight"]
    no = ["model.visual_model.image_encoder.blocks.0.attn.qkv.weight", "model.embed_tokens.weight", "model.norm.weight",
          "model.layers.0.input_layernorm.weight", "model.mm_projector.bias", "model.layers.0.self_attn.q_proj.bias",
          "model.vision_tower.vision_tower.vision_model.encoder.layers.0.self_attn.q_proj.weight"]
    assert all(quant.nf4_linear(n) for n in yes)
    assert not any(quant.nf4_linear(n) for n in no)
    assert not quant.nf4_linear("lm_head.weight", lm_head=False)
    gr, ur = quant.swiglu_rows(48)
    assert gr.tolist()[:17] == list(range(16)) + [32] and ur.tolist()[:2] == [16, 17]


def test_rope_row_map_inverts_rope_permute_rows():
    from haff import ops, quant
    w = torch.arange(768, dtype=torch.float32)[:, None].repeat(1, 2)
    perm = ops.rope_permute_rows(w)
    rmap = quant.rope_row_map(768, "cpu").long()
    out = torch.empty_like(w)
    out[rmap] = w
    assert torch.equal(out, perm)


def test_load_in_4bit_option_refusals():
    from haff import config as hcfg
    from haff.lisa import LisaMI355
    cfg = hcfg.tiny()
    with pytest.raises(ValueError, match="float16"):
        LisaMI355(cfg, {}, dtype=torch.bfloat16, load_in_4bit=True)
    with pytest.raises(ValueError, match="fp4"):
        LisaMI355(cfg, {}, dtype=torch.float16, load_in_4bit=True, bnb_4bit_quant_type="fp4")


def test_nf4_entry_points_declared():
    """(their host-side refusals: tests/test_quant_contract_cpu.py)"""
    text = open(os.path.join(ROOT, "include", "haff_hip.h")).read()
    for name in ("haff_nf4_quantize_f16", "haff_nf4_dequant_f16", "haff_gemm_nf4_f16"):
        assert re.search(r"^int " + name + r"\(", text, flags=re.M) and name in haff.EXPORTED_SYMBOLS
    if not os.path.exists(haff.LIB_PATH):
        haff.build_library()
    assert all(hasattr(ctypes.CDLL(haff.LIB_PATH), n) for n in ("haff_nf4_quantize_f16", "haff_nf4_dequant_f16", "haff_gemm_nf4_f16"))
