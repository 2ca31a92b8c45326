"""The 4-bit NF4 mode on the MI355X: the device quantiser and dequantiser bit for bit against the CPU restatement (tests/nf4_ref.py),
haff_gemm_nf4_f16 at the 7B / 13B decode shapes against haff_gemm_f16 on the dequantised weights, and LisaMI355(load_in_4bit=True)
against the oracle run on the dequantised weights."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/nf4_ref.py
import nf4_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu


def _cases():
    g = torch.Generator().manual_seed(11)
    gauss = (torch.randn(96, 640, generator=g) * 0.02).half()
    heavy = (torch.distributions.StudentT(2.0).sample((80, 512)) * 0.01).half()
    edge = (torch.randn(64, 256, generator=g) * 100).half()
    edge[0, 5], edge[3, 70], edge[7, 0] = 65504.0, -65504.0, 65504.0
    edge[9, :64] = 0.0                                                       # an all-zero block
    edge[10, 64:128] = (torch.randint(-1023, 1024, (64,), generator=g).float() * 2.0 ** -24).half()   # a block of subnormals only
    edge[11, :64] = -0.0
    return {"gauss": gauss, "heavy": heavy, "edges": edge}


def _check_quant(dev, w, dq):
    from haff import ops
    packed, absmax, off = ops.nf4_quantize(w.to(dev), double_quant=dq)
    off = off.cpu()
    rp, ra, _ = R.quantize(w, double_quant=dq, offset=off)
    mean = R.quantize(w, double_quant=False)[1].double().mean().item()
    assert abs(off.item() - mean) <= 1e-6 * abs(mean)
    assert torch.equal(packed.cpu(), rp)
    assert torch.equal(absmax.cpu().view(torch.int32), ra.view(torch.int32))
    return packed, absmax, rp, ra


@pytest.mark.parametrize("dq", [True, False])
@pytest.mark.parametrize("case", ["gauss", "heavy", "edges"])
def test_quantizer_and_dequant_bit_exact(dev, case, dq):
    from haff import ops
    w = _cases()[case]
    packed, absmax, rp, ra = _check_quant(dev, w, dq)
    got = ops.nf4_dequant(packed, absmax).cpu()
    assert torch.equal(got.view(torch.int16), R.dequant(rp, ra).view(torch.int16))
    if case == "edges":
        assert (got[9, :64] == 0).all() and (got[11, :64] == 0).all()


def test_quantizer_bit_exact_at_7b_shape(dev):
    w = (torch.randn(4096, 11008, generator=torch.Generator().manual_seed(3)) * 0.02).half()
    _check_quant(dev, w, True)


def test_row_maps_of_quantizer_and_dequant(dev):
    """q|k|v concatenation and the SwiGLU interleave through the quantiser's row map, the RoPE permutation through the dequantiser's:
    every stored row is the row quantised on its own."""
    from haff import ops, quant
    g = torch.Generator().manual_seed(4)
    H, F = 256, 512
    q, k, v = [(torch.randn(H, H, generator=g) * 0.02).half() for _ in range(3)]
    wq = quant.quantize([(q, None), (k, None), (v, None)], dev)
    ref = torch.cat([R.dequant(*R.quantize(t, offset=ops.nf4_quantize(t.to(dev))[2].cpu())[:2]) for t in (q, k, v)])
    assert torch.equal(wq.dequant().cpu().view(torch.int16), ref.view(torch.int16))
    perm = ops.rope_permute_rows(ref)
    got = wq.dequant(row_map=quant.rope_row_map(3 * H, dev)).cpu()
    assert torch.equal(got.view(torch.int16), perm.view(torch.int16))
    gate, up = [(torch.randn(F, H, generator=g) * 0.02).half() for _ in range(2)]
    gr, ur = quant.swiglu_rows(F)
    wgu = quant.quantize([(gate, gr), (up, ur)], dev).dequant().cpu()
    dg, du = [R.dequant(*R.quantize(t, offset=ops.nf4_quantize(t.to(dev))[2].cpu())[:2]) for t in (gate, up)]
    inter = torch.stack([dg.view(F // 16, 16, -1), du.view(F // 16, 16, -1)], dim=1).reshape(2 * F, -1)
    assert torch.equal(wgu.view(torch.int16), inter.view(torch.int16))


SHAPES = {   # name: (N, K, swiglu, out_f32)
    "7b_qkv": (3 * 4096, 4096, False, False), "7b_o": (4096, 4096, False, False), "7b_gu": (2 * 11008, 4096, True, False),
    "7b_down": (4096, 11008, False, False), "7b_lm_head": (32003, 4096, False, True),
    "13b_qkv": (3 * 5120, 5120, False, False), "13b_gu": (2 * 13824, 5120, True, False), "13b_down": (5120, 13824, False, False),
}


@pytest.mark.parametrize("M", [1, 2, 8, 16, 33, 64])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_gemm_nf4_matches_f16_product_on_dequantised_weights(dev, shape, M):
    from haff import ops, quant
    N, K, swiglu, out_f32 = SHAPES[shape]
    g = torch.Generator(device=dev).manual_seed(M * 7 + N)
    w = quant.quantize([(torch.randn(N, K, device=dev, generator=g) * 0.02, None)], dev)
    wd = w.dequant()
    x = torch.randn(M, K, device=dev, generator=g).half()
    bias = torch.randn(N, device=dev, generator=g) * 0.1
    od = torch.float32 if out_f32 else torch.float16
    got = ops.linear_nf4(x, w.packed, w.absmax, bias=bias, swiglu=swiglu, out_dtype=od)
    ref = ops.linear(x, wd, bias=bias, swiglu=swiglu, out_dtype=od)
    again = ops.linear_nf4(x, w.packed, w.absmax, bias=bias, swiglu=swiglu, out_dtype=od)
    assert torch.equal(got.view(torch.int16 if od == torch.float16 else torch.int32),
                       again.view(torch.int16 if od == torch.float16 else torch.int32))   # repeat runs bitwise equal
    mag = x.float().abs() @ wd.float().abs().T + bias.abs()
    if swiglu:   # bound of the SwiGLU output from the gate / up magnitudes: compare the pre-activation products instead
        pre = ops.linear_nf4(x, w.packed, w.absmax, bias=bias, out_dtype=torch.float32)
        pre_ref = ops.linear(x, wd, bias=bias, out_dtype=torch.float32)
        assert ((pre - pre_ref).abs() <= 1e-5 * mag).all()
        assert torch.allclose(got.float(), ref.float(), rtol=4e-3, atol=1e-3)
        return
    tol = 1e-5 * mag
    if od == torch.float16:
        tol = tol + (ref.float().abs() * 2.0 ** -10).clamp_min(2.0 ** -24)
    assert ((got.float() - ref.float()).abs() <= tol).all(), (got.float() - ref.float()).abs().max().item()
    if shape == "7b_o":   # the residual may alias C
        r = torch.randn(M, N, device=dev, generator=g).half()
        c = r.clone()
        ops.linear_nf4(x, w.packed, w.absmax, resid=c, out=c)
        ref2 = ops.linear(x, wd, resid=r.clone(), out=r.clone())
        assert ((c.float() - ref2.float()).abs() <= 1e-5 * mag + (ref2.float().abs() * 2.0 ** -10).clamp_min(2.0 ** -24) + 1e-3).all()


# ---- model level --------------------------------------------------------------------------------------------------------------
def _deq_state_dict(sd, dev, lm_head=True):
    from haff import quant
    out = dict(sd)
    for k, v in sd.items():
        if quant.nf4_linear(k, lm_head=lm_head):
            out[k] = quant.round_trip(v, dev).float().cpu()
    return out


def _iou(a, b):
    inter = (a & b).sum().item()
    union = (a | b).sum().item()
    return inter / union if union else 1.0


@pytest.mark.parametrize("cfg_name", ["tiny", "mid"])
def test_load_in_4bit_matches_oracle_on_dequantised_weights(dev, cfg_name):
    import test_fp16_lisa_gpu as F16
    from haff.lisa import LisaMI355
    from oracle import lisa_oracle as O
    cfg, sd, images, images_clip, ids, forced = F16._setup(cfg_name)
    sdq = _deq_state_dict(sd, dev)
    S = cfg.sam.img_size
    B = ids.shape[0]
    resize = [(S, S), (S, S - 32)]
    orig = [(S, S), (S // 2 + 3, S // 2 - 10)]
    with torch.no_grad():
        ref_ids, ref_l, ref_r, ref_t = O.lisa_evaluate(sdq, cfg, images_clip, images, ids, resize, orig,
                                                       max_new_tokens=forced.shape[1], forced_answer=forced, use_cache=False)
    stats = {}
    for name, model in (("nf4", lambda: LisaMI355(cfg, sd, dtype=torch.float16, device=dev, load_in_4bit=True)),
                        ("bf16", lambda: LisaMI355(cfg, sdq, dtype=torch.bfloat16, device=dev))):
        m = model()
        out_ids, left, right, tax = F16._run(m, dev, images_clip, images, ids, forced, resize, orig)
        errs, ious, terrs = [], [], []
        for i in range(B):
            for got, ref in ((left[i], ref_l[i]), (right[i], ref_r[i])):
                gg = got.cpu()
                assert torch.isfinite(gg).all()
                errs.append((gg - ref).abs().max().item() / ref.abs().max().item())
                ious.append(_iou(gg > 0, ref > 0))
            terrs.append((tax[i].cpu() - ref_t[i]).abs().max().item())
        stats[name] = (out_ids.cpu(), max(errs), min(ious), max(terrs))
        print(f"{cfg_name} {name}: max err/scale {max(errs):.3e}, min IoU {min(ious):.5f}, taxonomy err {max(terrs):.3e}")
        del m
    ids4, err4, iou4, terr4 = stats["nf4"]
    _, err_bf, iou_bf, _ = stats["bf16"]
    assert torch.equal(ids4, ref_ids)
    assert err4 <= 0.5 * err_bf, (err4, err_bf)
    assert iou4 >= iou_bf, (iou4, iou_bf)
    assert terr4 <= 1e-3


def test_quantisation_is_applied_and_footprint(dev):
    """The 4-bit model's logits differ from the fp16 model's on the original weights by far more than from the fp16 model on the
    dequantised weights (fp16 noise), and its Llama + lm_head bytes are <= 0.30x the fp16 model's."""
    import test_fp16_lisa_gpu as F16
    from haff.lisa import LisaMI355
    cfg, sd, *_ = F16._setup("mid")
    sdq = _deq_state_dict(sd, dev)
    x = torch.randn((2, 40, cfg.llm.hidden), generator=torch.Generator().manual_seed(1)).half().to(dev)
    logits = {}
    bytes_ = {}
    for name, s, q4 in (("nf4", sd, True), ("f16", sd, False), ("f16_deq", sdq, False)):
        m = LisaMI355(cfg, s, dtype=torch.float16, device=dev, load_in_4bit=q4)
        cache = m.llm.new_cache(2, 48)
        h = m.llm.forward(x.clone(), cache)   # (forward adds the residuals into its input)
        logits[name] = m.llm.next_token_logits(h[:, -1].contiguous()).float().cpu()
        bytes_[name] = m.llm_weight_bytes()
        del m
    d_quant = (logits["nf4"] - logits["f16"]).abs().max().item()
    d_noise = (logits["nf4"] - logits["f16_deq"]).abs().max().item()
    print(f"logit diff vs fp16 on original weights {d_quant:.3e}, vs fp16 on dequantised weights {d_noise:.3e}; "
          f"bytes {bytes_['nf4']} / {bytes_['f16']}")
    assert d_quant > 10 * d_noise
    assert bytes_["nf4"] <= 0.30 * bytes_["f16"]


@pytest.mark.parametrize("B", [1, 8])
def test_graph_decode_equals_eager_in_4bit_mode(dev, B):
    import test_fp16_lisa_gpu as F16
    from haff.lisa import LisaMI355
    cfg, sd, images, images_clip, ids, forced = F16._setup("mid", B=B)
    S = cfg.sam.img_size
    resize, orig = [(S, S)] * B, [(S, S)] * B
    model = LisaMI355(cfg, sd, dtype=torch.float16, device=dev, load_in_4bit=True)
    runs = []
    for graphs in (True, False):
        model.decode_graphs = graphs
        out = F16._run(model, dev, images_clip, images, ids, forced, resize, orig)
        runs.append(out)
    assert torch.equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1] + runs[0][2], runs[1][1] + runs[1][2]):
        assert torch.equal(a, b)
    # and the decode hidden states themselves: generate() with graphs vs eager
    model.decode_graphs = True
    _, h1 = model.generate(images_clip.to(dev), ids.to(dev), max_new_tokens=4, forced_answer=forced.to(dev))
    model.decode_graphs = False
    _, h2 = model.generate(images_clip.to(dev), ids.to(dev), max_new_tokens=4, forced_answer=forced.to(dev))
    assert torch.equal(h1.view(torch.int16), h2.view(torch.int16))


@pytest.mark.parametrize("width", ["7b", "13b"])
def test_full_width_llama_layer_in_4bit_mode_matches_oracle(dev, width):
    """One Llama layer + final norm at 7B / 13B width, prefill of 291 positions (2 rows: the dequantise-then-f16 path, fused q|k|v
    RoPE) then two cached steps (the NF4 product), against the oracle's llama_forward on the dequantised weights."""
    import haff  # noqa: F401
    from haff import config as hcfg
    from haff import weights as hw
    from haff.llava import LlamaHip
    from oracle import lisa_oracle as O
    cfg = hcfg.haff_7b() if width == "7b" else hcfg.haff_13b()
    cfg.llm.layers = 1
    shapes = {k: v for k, v in hw.llm_shapes(cfg).items() if k.startswith("model.layers.") or k == "model.norm.weight"}
    shapes["model.embed_tokens.weight"] = (8, cfg.llm.hidden)
    shapes["lm_head.weight"] = (64, cfg.llm.hidden)
    sd = hw.make_state_dict(cfg, 31, shapes)
    sdq = _deq_state_dict(sd, dev)
    B, T, Hd = 2, 291, cfg.llm.hidden
    x = torch.randn((B, T + 2, Hd), generator=torch.Generator().manual_seed(2)).half().float()
    with torch.no_grad():
        ref = O.llama_forward(sdq, x, cfg.llm)
    for fused in (True, "force"):
        llm = LlamaHip(sd, cfg.llm, torch.float16, dev, nf4=True)
        llm.fused_qkv_rope = fused
        cache = llm.new_cache(B, T + 2)
        xd = x.to(dev, torch.float16)
        got = [llm.forward(xd[:, :T].contiguous(), cache)]
        for s in range(2):
            got.append(llm.forward(xd[:, T + s:T + s + 1].contiguous(), cache))
        got = torch.cat(got, 1).float().cpu()
        err = (got - ref).abs().max().item() / ref.abs().max().item()
        print(f"llama {width} nf4 (fused {fused}): hidden rel err {err:.3e}")
        assert err <= 1.5e-2
        del llm
