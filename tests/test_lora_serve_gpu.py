"""Serving LoRA adapters unmerged on the NF4 base, on the MI355X: haff_nf4_dequant_lora_f16 bit for bit and haff_gemm_nf4_lora_f16
within its tolerance against the CPU restatement (tests/lora_serve_ref.py), the 7B shapes against the composed route (plain NF4
product, ops.linear for t, haff_lora_out_f16), LisaMI355(load_in_4bit=True, lora_state=) and one full-width Llama layer against the
oracle on the effective weights deq(Q(W)) + s B A, graph decode against eager, and a train_ds.py --load_in_4bit checkpoint."""
import math
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/nf4_ref.py, tests/lora_serve_ref.py
import lora_serve_ref as LR   # noqa: E402
import nf4_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu

ALL7 = "q_proj,k_proj,v_proj,o_proj,gate_proj,up_proj,down_proj"


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == torch.float16 else torch.int32)


def _lora(dev, c):
    from haff import quant
    return quant.Nf4Lora(c["a_cat"].to(dev), c["b"].to(dev), c["nseg"], c["seg_rows"], c["scale"])


# ---- kernel 1: the dequantisation with the rank update folded in, bit for bit ----------------------------------------------------
@pytest.mark.parametrize("nseg,seg_rows", [(1, 16), (1, 32), (2, 16), (2, 32), (3, 16), (3, 32)])
@pytest.mark.parametrize("N,K", [(16, 64), (48, 192), (96, 448)])
def test_dequant_lora_bit_exact(dev, N, K, nseg, seg_rows):
    from haff import ops
    c = LR.make_case(1, N, K, nseg, seg_rows, 31 * N + nseg + seg_rows)
    want = LR.dequant_lora(c["packed"], c["absmax"], c["a_cat"], c["b"], nseg, seg_rows, c["scale"])
    assert not torch.equal(_bits(want), _bits(c["wdeq"]))
    packed, absmax, L = c["packed"].to(dev), c["absmax"].to(dev), _lora(dev, c)
    got = ops.nf4_dequant_lora(packed, absmax, L)
    assert torch.equal(_bits(got.cpu()), _bits(want))
    # ldo > K: the columns past K are left alone
    wide = torch.full((N, K + 24), 7.0, dtype=torch.float16, device=dev)
    ops.nf4_dequant_lora(packed, absmax, L, out=wide[:, :K])
    assert torch.equal(_bits(wide[:, :K].cpu()), _bits(want)) and (wide[:, K:] == 7.0).all()


def test_dequant_lora_rope_map_zero_segment_and_padded_rank(dev):
    from haff import ops, quant
    N, K, H = 768, 256, 256
    # q and v adapted at rank 4 (zero-padded), k not: the q | k | v layout of the default --lora_target_modules
    c = LR.make_case(1, N, K, 3, H, 5, r=4, zero_seg=1)
    assert (c["a_cat"][4:8] == 0).all() and (c["b"][:, 4:] == 0).all()
    want = LR.dequant_lora(c["packed"], c["absmax"], c["a_cat"], c["b"], 3, H, c["scale"])
    packed, absmax, L = c["packed"].to(dev), c["absmax"].to(dev), _lora(dev, c)
    got = ops.nf4_dequant_lora(packed, absmax, L).cpu()
    assert torch.equal(_bits(got), _bits(want))
    plain = ops.nf4_dequant(packed, absmax).cpu()
    assert torch.equal(_bits(got[H:2 * H]), _bits(plain[H:2 * H]))            # the segment without adapter: the plain kernel's bits
    assert not torch.equal(_bits(got[:H]), _bits(plain[:H])) and not torch.equal(_bits(got[2 * H:]), _bits(plain[2 * H:]))
    # the RoPE row permutation of the fused q | k | v prefill, through the same output row map as the plain dequantisation
    rmap = quant.rope_row_map(N, dev)
    got_r = ops.nf4_dequant_lora(packed, absmax, L, row_map=rmap).cpu()
    assert torch.equal(_bits(got_r), _bits(ops.rope_permute_rows(want)))


# ---- kernel 2: the streamed product with the rank update in its epilogue -------------------------------------------------------
def _linear_lora(dev, c, **kw):
    from haff import ops
    return ops.linear_nf4(c["x"].to(dev), c["packed"].to(dev), c["absmax"].to(dev), lora=_lora(dev, c), lora_t=c["t"].to(dev), **kw)


def _ref_tol(c, out_dtype, bias=None):
    a = (c["t"], c["b"], c["nseg"], c["seg_rows"], c["scale"])
    ref = LR.product_lora(c["x"], c["packed"], c["absmax"], *a, bias=bias)
    return ref, LR.tol(c["x"], c["wdeq"], bias, out_dtype, *a, ref=ref)


@pytest.mark.parametrize("N", [48, 96])
@pytest.mark.parametrize("K", [64, 448, 4096])
@pytest.mark.parametrize("M", [1, 16, 17, 33, 64])
def test_gemm_nf4_lora_matches_restatement(dev, M, K, N):
    """K = 64 and 448: 1 and 7 blocks for 8 waves, so some waves own no block. Three segments of 16 rows: every 16-row tile of a
    workgroup has another segment."""
    c = LR.make_case(M, N, K, 3, 16, 1000 * M + K + N)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(M)) * 0.1
    ref, tol = _ref_tol(c, torch.float16, bias)
    got = _linear_lora(dev, c, bias=bias.to(dev))
    again = _linear_lora(dev, c, bias=bias.to(dev))
    assert torch.equal(_bits(got), _bits(again))                              # repeat runs bitwise equal
    err = (got.cpu().double() - ref).abs()
    print(f"M {M} K {K} N {N}: max err / tol {(err / tol).max().item():.3f}")
    assert (err <= tol).all()
    # the update is what is being tested: the plain product lies far outside
    plain = R.product(c["x"], c["packed"], c["absmax"], bias)
    assert ((plain - ref).abs() > tol).double().mean().item() > 0.9


@pytest.mark.parametrize("M", [1, 17, 64])
def test_gemm_nf4_lora_f32_output_residual_alias_and_row_map(dev, M):
    N, K = 96, 448
    c = LR.make_case(M, N, K, 2, 16, 77 + M)
    ref, tol = _ref_tol(c, torch.float32)
    got = _linear_lora(dev, c, out_dtype=torch.float32)
    assert got.dtype == torch.float32 and ((got.cpu().double() - ref).abs() <= tol).all()
    # the residual aliasing the output
    g = torch.Generator().manual_seed(M)
    r = torch.randn(M, N, generator=g).half()
    buf = r.to(dev)
    _linear_lora(dev, c, resid=buf, out=buf)
    ref_r = ref + r.double()
    tol_r = LR.tol(c["x"], c["wdeq"], None, torch.float16, c["t"], c["b"], 2, 16, c["scale"], ref=ref_r) + 2.0 ** -24 * r.double().abs()
    assert ((buf.cpu().double() - ref_r).abs() <= tol_r).all()
    # a row map with dropped rows: row m goes to out row 2 (M - 1 - m), every third row nowhere
    rmap = torch.tensor([-1 if m % 3 == 1 else 2 * (M - 1 - m) for m in range(M)], dtype=torch.int32)
    out = torch.full((2 * M, N), 3.0, dtype=torch.float16, device=dev)
    _linear_lora(dev, c, row_map=rmap.to(dev), out=out)
    out = out.cpu()
    ref16, tol16 = _ref_tol(c, torch.float16)
    written = torch.zeros(2 * M, dtype=torch.bool)
    for m in range(M):
        if rmap[m] >= 0:
            written[rmap[m]] = True
            assert ((out[rmap[m]].double() - ref16[m]).abs() <= tol16[m]).all()
    assert (out[~written] == 3.0).all()


def _swiglu_ref(pre, tol_pre):
    """silu(gate) * up of the [gate x16 | up x16] interleave in float64, and the tolerance that follows from the pre-activations':
    |d silu| <= 1.1 |d gate|; plus 2^-18 of the result for the kernel's exp / reciprocal approximations (a few fp32 ulps each)."""
    M, N = pre.shape
    p, t = pre.view(M, N // 32, 2, 16), tol_pre.view(M, N // 32, 2, 16)
    g, u, tg, tu = p[:, :, 0], p[:, :, 1], t[:, :, 0], t[:, :, 1]
    silu = g / (1 + torch.exp(-g))
    ref = (silu * u).reshape(M, N // 2)
    tol = (1.1 * tg * u.abs() + silu.abs() * tu + 1.1 * tg * tu).reshape(M, N // 2) + 2.0 ** -18 * ref.abs()
    return ref, tol


@pytest.mark.parametrize("M", [1, 16, 33, 64])
@pytest.mark.parametrize("N,K", [(96, 448), (64, 4096)])
def test_gemm_nf4_lora_swiglu_two_segments(dev, M, N, K):
    c = LR.make_case(M, N, K, 2, 16, 9 * M + N)
    pre, tol_pre = _ref_tol(c, torch.float32)
    got_pre = _linear_lora(dev, c, out_dtype=torch.float32).cpu().double()
    assert ((got_pre - pre).abs() <= tol_pre).all()
    ref, tol = _swiglu_ref(pre, tol_pre - pre.abs() * 2.0 ** -23)             # (without the fp32 output rounding of the line above)
    tol = tol + ref.abs().clamp_min(2.0 ** -14) * 2.0 ** -10                  # the f16 output
    got = _linear_lora(dev, c, swiglu=True)
    assert got.shape == (M, N // 2) and torch.equal(_bits(got), _bits(_linear_lora(dev, c, swiglu=True)))
    assert ((got.cpu().double() - ref).abs() <= tol).all()
    plain, _ = _swiglu_ref(R.product(c["x"], c["packed"], c["absmax"]), tol_pre)
    assert ((plain - ref).abs() > tol).double().mean().item() > 0.8


def _composed(dev, x, w, L, M):
    """The composed route, fp32 [M, N]: the plain NF4 product, t = linear(x, a_cat), and haff_lora_out_f16 once per segment on a
    zero f16 buffer with the other segments' coefficients zeroed (each element is rounded to f16 once; adding 0 is exact)."""
    from haff import ops
    from haff.lib import check, load_library
    lib = load_library()
    N = w.shape[0]
    y = ops.linear_nf4(x, w.packed, w.absmax, out_dtype=torch.float32)
    t = ops.linear(x, L.a_cat)
    z = torch.zeros((M, N), dtype=torch.float16, device=dev)
    seg = ((torch.arange(N, device=dev) // L.seg_rows) % L.nseg)
    Mp = (M + 3) // 4 * 4
    for s in range(L.nseg):
        tT = torch.zeros((8, Mp), dtype=torch.float16, device=dev)
        tT[:, :M] = t[:, 8 * s:8 * s + 8].T
        bs = (L.b * (seg == s)[:, None]).contiguous()
        check(lib.haff_lora_out_f16(tT.data_ptr(), tT.stride(0), bs.data_ptr(), z.data_ptr(), z.stride(0), M, N, float(L.scale),
                                    torch.cuda.current_stream().cuda_stream), "haff_lora_out_f16")
    return y, z, t


@pytest.mark.parametrize("M", [1, 64])
@pytest.mark.parametrize("proj", ["qkv", "gu", "down"])
def test_gemm_nf4_lora_7b_shapes_match_the_composed_route(dev, proj, M):
    """7B q | k | v, gate | up (SwiGLU) and down through ops.linear_nf4(lora=) with t from its own ops.linear launch. Both routes run the
    same K loop, so their x deq(W)^T sums are the same bits; what may differ is the rank update: the MFMA's fp32 sum against
    haff_lora_out_f16's fma chain rounded to f16 (2^-11 relative), each within 2^-16 of sum |t B|."""
    from haff import ops, quant
    H, F = 4096, 11008
    N, K, nseg, seg_rows, swiglu = {"qkv": (3 * H, H, 3, H, False), "gu": (2 * F, H, 2, 16, True), "down": (H, F, 1, 16, False)}[proj]
    g = torch.Generator(device=dev).manual_seed(M + N)
    w = quant.quantize([(torch.randn(N, K, device=dev, generator=g) * 0.02, None)], dev)
    x = torch.randn(M, K, device=dev, generator=g).half()
    a_cat = ((torch.rand((8 * nseg, K), device=dev, generator=g) * 2 - 1) / math.sqrt(K)).half()
    b = ((torch.rand((N, 8), device=dev, generator=g) * 2 - 1) * 0.05).half()
    L = quant.Nf4Lora(a_cat, b, nseg, seg_rows, 2.0)
    y, z, t = _composed(dev, x, w, L, M)
    seg = ((torch.arange(N, device=dev) // seg_rows) % nseg)
    rows = 8 * seg[:, None] + torch.arange(8, device=dev)[None, :]
    mag_u = 2.0 * torch.einsum("mnj,nj->mn", t.double().abs()[:, rows], b.double().abs())
    pre = ops.linear_nf4(x, w.packed, w.absmax, lora=L, out_dtype=torch.float32)
    comp = y.double() + z.double()
    tol_pre = (2 * R.C_ACC + 2.0 ** -11) * mag_u + comp.abs() * 2.0 ** -22
    d = (pre.double() - comp).abs()
    print(f"{proj} M {M}: max err / tol {(d / tol_pre).max().item():.3f}; |update| / |tol| {(z.double().norm() / tol_pre.norm()).item():.1f}")
    assert (d <= tol_pre).all()
    assert (z.double().abs() > tol_pre).double().mean().item() > 0.95         # dropping the update could not pass
    got = ops.linear_nf4(x, w.packed, w.absmax, lora=L, swiglu=swiglu)
    assert torch.equal(_bits(got), _bits(ops.linear_nf4(x, w.packed, w.absmax, lora=L, swiglu=swiglu)))
    if swiglu:
        ref, tol = _swiglu_ref(comp, tol_pre)
    else:
        ref, tol = comp, tol_pre
    tol = tol + ref.abs().clamp_min(2.0 ** -14) * 2.0 ** -10
    assert ((got.double() - ref).abs() <= tol).all()


# ---- model level ----------------------------------------------------------------------------------------------------------------
def _trained(cfg, sd, seed, targets=ALL7):
    """A synthetic LisaTrainable.state_dict(): adapters on `targets` (init_lora's distributions, B non-zero, f16 values) and the
    tensors the trainer trains in full, moved away from the base's by 2 % of their spread."""
    from haff import train_model as TM
    g = torch.Generator().manual_seed(seed)
    st = {k: v.half().float() for k, v in TM.init_lora(cfg, TM.lora_targets(cfg, targets), 8, seed, init_b_zero=False).items()}
    full = ["model.embed_tokens.weight", "lm_head.weight"] + [k for k in sd if "text_hidden_fcs" in k] + \
        [k for k in sd if k.startswith(TM.V + ".mask_decoder_left.") or k.startswith(TM.V + ".mask_decoder_right.")]
    for k in full:
        v = sd[k].float()
        spread = v.std() if v.numel() > 1 else v.abs().max()
        st[k] = (v + 0.02 * spread * torch.randn(v.shape, generator=g)).half().float()
    return st


def _effective_state_dict(sd, st, dev, scale=2.0):
    """What LisaMI355(load_in_4bit=True, lora_state=st) computes with, as fp32 tensors for the oracle: the trained full tensors,
    the trainer's NF4 set round-tripped, and deq(Q(W)) + s B A on the adapted projections."""
    from haff import quant
    from haff import train_model as TM
    out = dict(sd)
    out.update({k: v for k, v in st.items() if ".lora_" not in k})
    for k in list(out):
        if TM.nf4_frozen_linear(k):
            out[k] = quant.round_trip(out[k], dev).float().cpu()
    for k in [k for k in st if k.endswith(".lora_A")]:
        mod = k[:-len(".lora_A")]
        out[mod + ".weight"] = out[mod + ".weight"] + scale * (st[mod + ".lora_B"].float() @ st[k].float())
    return out


def _score(model, dev, args, refs):
    import test_fp16_lisa_gpu as F16
    _iou = F16._iou
    (ref_ids, ref_l, ref_r, ref_t) = refs
    out_ids, left, right, tax = F16._run(model, dev, *args)
    errs, ious, terrs = [], [], []
    for i in range(len(left)):
        for got, ref in ((left[i], ref_l[i]), (right[i], ref_r[i])):
            gg = got.cpu()
            assert torch.isfinite(gg).all()
            errs.append((gg - ref).abs().max().item() / ref.abs().max().item())
            ious.append(_iou(gg > 0, ref > 0))
        terrs.append((tax[i].cpu() - ref_t[i]).abs().max().item())
    return out_ids.cpu(), max(errs), min(ious), max(terrs)


@pytest.mark.parametrize("cfg_name", ["tiny", "mid"])
def test_unmerged_adapters_match_oracle_on_effective_weights(dev, cfg_name):
    """The pattern and the bounds of test_load_in_4bit_matches_oracle_on_dequantised_weights, with adapters on all seven projections
    and the trained full tensors overlaid; the oracle runs on deq(Q(W)) + s B A. Beside it the only route that existed before:
    merge_lora.merge_state_dict into the 16-bit weights, then load_in_4bit=True (which quantises W + s B A again, and lm_head and
    text_hidden_fcs with it): further from the function the trainer optimised."""
    import test_fp16_lisa_gpu as F16
    from haff import merge_lora
    from haff.lisa import LisaMI355
    from oracle import lisa_oracle as O
    cfg, sd, images, images_clip, ids, forced = F16._setup(cfg_name)
    st = _trained(cfg, sd, 17)
    eff = _effective_state_dict(sd, st, dev)
    S = cfg.sam.img_size
    resize = [(S, S), (S, S - 32)]
    orig = [(S, S), (S // 2 + 3, S // 2 - 10)]
    with torch.no_grad():
        refs = O.lisa_evaluate(eff, cfg, images_clip, images, ids, resize, orig, max_new_tokens=forced.shape[1], forced_answer=forced,
                               use_cache=False)
    args = (images_clip, images, ids, forced, resize, orig)
    merged = merge_lora.merge_state_dict(sd, st, 8, 16, torch.float16)
    merged.update({k: v for k, v in sd.items() if k not in merged})
    stats = {}
    for name, make in (("unmerged", lambda: LisaMI355(cfg, sd, dtype=torch.float16, device=dev, load_in_4bit=True, lora_state=st)),
                       ("bf16", lambda: LisaMI355(cfg, eff, dtype=torch.bfloat16, device=dev)),
                       ("requantised", lambda: LisaMI355(cfg, merged, dtype=torch.float16, device=dev, load_in_4bit=True))):
        m = make()
        if name == "unmerged":
            assert all(L[k].lora is not None for L in m.llm.layers for k in ("wqkv", "wo", "wgu", "wd")) and m.llm.lora_bytes() > 0
            assert isinstance(m.llm.lm_head, torch.Tensor)                   # the trainer's quantised set: lm_head stays f16
        stats[name] = _score(m, dev, args, refs)
        print(f"{cfg_name} {name}: max err/scale {stats[name][1]:.3e}, min IoU {stats[name][2]:.5f}, taxonomy err {stats[name][3]:.3e}")
        del m
    ids4, err4, iou4, terr4 = stats["unmerged"]
    _, err_bf, iou_bf, _ = stats["bf16"]
    assert torch.equal(ids4, refs[0])
    assert err4 <= 0.5 * err_bf, (err4, err_bf)
    assert iou4 >= iou_bf, (iou4, iou_bf)
    assert terr4 <= 1e-3
    assert stats["requantised"][1] > err4, (stats["requantised"][1], err4)


@pytest.mark.parametrize("width", ["7b", "13b"])
def test_full_width_llama_layer_with_unmerged_adapters_matches_oracle(dev, width):
    """test_full_width_llama_layer_in_4bit_mode_matches_oracle with adapters on all seven projections: a prefill of 2 x 291 rows
    (haff_nf4_dequant_lora_f16 in front of the f16 products, the fused q | k | v + RoPE among them) and two cached steps
    (haff_gemm_nf4_lora_f16), against llama_forward on the effective weights. The same bound."""
    import haff  # noqa: F401
    from haff import config as hcfg
    from haff import quant
    from haff import train_model as TM
    from haff import weights as hw
    from haff.llava import LlamaHip
    from oracle import lisa_oracle as O
    cfg = hcfg.haff_7b() if width == "7b" else hcfg.haff_13b()
    cfg.llm.layers = 1
    shapes = {k: v for k, v in hw.llm_shapes(cfg).items() if k.startswith("model.layers.") or k == "model.norm.weight"}
    shapes["model.embed_tokens.weight"] = (8, cfg.llm.hidden)
    shapes["lm_head.weight"] = (64, cfg.llm.hidden)
    sd = hw.make_state_dict(cfg, 31, shapes)
    st = {k: v.half().float() for k, v in TM.init_lora(cfg, TM.lora_targets(cfg, ALL7), 8, 3, init_b_zero=False).items()}
    pairs, r = quant.lora_pairs(st, cfg)
    assert r == 8 and len(pairs) == 7
    eff = _effective_state_dict(sd, st, dev)
    plain = _effective_state_dict(sd, {}, dev)
    B, T, Hd = 2, 291, cfg.llm.hidden
    x = torch.randn((B, T + 2, Hd), generator=torch.Generator().manual_seed(2)).half().float()
    with torch.no_grad():
        ref = O.llama_forward(eff, x, cfg.llm)
        ref_plain = O.llama_forward(plain, x, cfg.llm)
    moved = (ref_plain - ref).abs().max().item() / ref.abs().max().item()
    assert moved > 3 * 1.5e-2, moved                                          # without the adapters the bound below is missed
    for fused in (True, "force"):
        llm = LlamaHip(sd, cfg.llm, torch.float16, dev, nf4=True, lora=pairs, lora_scale=16 / r)
        llm.fused_qkv_rope = fused
        cache = llm.new_cache(B, T + 2)
        xd = x.to(dev, torch.float16)
        got = [llm.forward(xd[:, :T].contiguous(), cache)]
        for s in range(2):
            got.append(llm.forward(xd[:, T + s:T + s + 1].contiguous(), cache))
        got = torch.cat(got, 1).float().cpu()
        err = (got - ref).abs().max().item() / ref.abs().max().item()
        print(f"llama {width} nf4 + adapters (fused {fused}): hidden rel err {err:.3e}; the adapters move it by {moved:.3e}")
        assert err <= 1.5e-2
        del llm


@pytest.mark.parametrize("B", [1, 8])
def test_graph_decode_equals_eager_with_adapters(dev, B):
    import test_fp16_lisa_gpu as F16
    from haff.lisa import LisaMI355
    cfg, sd, images, images_clip, ids, forced = F16._setup("mid", B=B)
    S = cfg.sam.img_size
    resize, orig = [(S, S)] * B, [(S, S)] * B
    model = LisaMI355(cfg, sd, dtype=torch.float16, device=dev, load_in_4bit=True, lora_state=_trained(cfg, sd, 4))
    runs = []
    for graphs in (True, False):
        model.decode_graphs = graphs
        runs.append(F16._run(model, dev, images_clip, images, ids, forced, resize, orig))
    assert torch.equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1] + runs[0][2], runs[1][1] + runs[1][2]):
        assert torch.equal(a, b)
    model.decode_graphs = True
    _, h1 = model.generate(images_clip.to(dev), ids.to(dev), max_new_tokens=4, forced_answer=forced.to(dev))
    _, h1b = model.generate(images_clip.to(dev), ids.to(dev), max_new_tokens=4, forced_answer=forced.to(dev))   # a replay
    model.decode_graphs = False
    _, h2 = model.generate(images_clip.to(dev), ids.to(dev), max_new_tokens=4, forced_answer=forced.to(dev))
    assert torch.equal(_bits(h1), _bits(h2)) and torch.equal(_bits(h1b), _bits(h2))
    # ... and the adapters are in those hidden states
    base = LisaMI355(cfg, sd, dtype=torch.float16, device=dev, load_in_4bit=True, nf4_lm_head=False)
    _, h0 = base.generate(images_clip.to(dev), ids.to(dev), max_new_tokens=4, forced_answer=forced.to(dev))
    assert not torch.equal(_bits(h0), _bits(h2))


def test_train_ds_checkpoint_loads_through_lora_checkpoint(dev, tmp_path, capsys):
    """train_ds.py --load_in_4bit (tiny, synthetic) writes latest.pt; from_pretrained(load_in_4bit=True, lora_checkpoint=) serves it,
    equal to the constructor with lora_state=; a 16-bit fine-tune's checkpoint is refused by name before anything is loaded."""
    import test_fp16_lisa_gpu as F16
    from safetensors.torch import save_file
    import haff  # noqa: F401
    from haff import checkpoint, config as hcfg, merge_lora as ML, train_ds
    from haff.lisa import LisaMI355
    common = ["--synthetic", "tiny", "--grad_accumulation_steps", "1", "--batch_size", "2", "--mask_hw", "64", "48", "--lora_dropout", "0",
              "--no_eval", "--lr", "0.0003", "--precision", "fp16", "--print_freq", "1", "--log_base_dir", str(tmp_path),
              "--epochs", "1", "--steps_per_epoch", "2"]
    train_ds.main(common + ["--exp_name", "q", "--load_in_4bit"])
    train_ds.main(common + ["--exp_name", "h"])
    capsys.readouterr()
    path, path16 = [tmp_path / n / "ckpt_model" / "latest.pt" for n in ("q", "h")]
    blob = torch.load(path, map_location="cpu", weights_only=False)
    assert blob["base_format"] == "nf4"
    cfg = hcfg.tiny()
    sd = {k: v.cpu() for k, v in checkpoint.synthetic_state_dict(cfg, 1234, dev, torch.float16).items()}
    vdir, clip = tmp_path / "base", tmp_path / "clip"
    clip.mkdir()
    ML.save_pretrained({k: v.contiguous() for k, v in sd.items() if "vision_tower" not in k}, str(vdir), ML.hf_config(cfg, torch.float16))
    pfx = "model.vision_tower.vision_tower."
    save_file({k[len(pfx):]: v.contiguous() for k, v in sd.items() if k.startswith(pfx)}, str(clip / "model.safetensors"))
    with pytest.raises(ValueError, match=r"latest\.pt.*base_format=None.*merge_lora"):
        LisaMI355.from_pretrained(str(vdir), vision_tower=str(clip), torch_dtype=torch.float16, device=dev, load_in_4bit=True,
                                  lora_checkpoint=str(path16))
    with pytest.raises(ValueError, match=r"needs load_in_4bit=True"):
        LisaMI355.from_pretrained(str(vdir), vision_tower=str(clip), torch_dtype=torch.float16, device=dev, lora_checkpoint=str(path))
    m1 = LisaMI355.from_pretrained(str(vdir), vision_tower=str(clip), torch_dtype=torch.float16, device=dev, load_in_4bit=True,
                                   lora_checkpoint=str(path), lora_alpha=16)
    adapted = [L["wqkv"].lora for L in m1.llm.layers]
    assert all(a is not None and a.nseg == 3 and a.scale == 2.0 for a in adapted)
    assert all(bool((a.b[:cfg.llm.hidden] != 0).any()) and bool((a.b[cfg.llm.hidden:2 * cfg.llm.hidden] == 0).all()) for a in adapted)   # q trained, k none
    assert all(L[k].lora is None for L in m1.llm.layers for k in ("wo", "wgu", "wd"))
    assert torch.equal(m1.llm.embed.cpu(), blob["params"]["model.embed_tokens.weight"].half())
    m2 = LisaMI355(cfg, sd, dtype=torch.float16, device=dev, load_in_4bit=True, lora_state=blob["params"])
    _, _, images, images_clip, ids, forced = F16._setup("tiny")
    S = cfg.sam.img_size
    outs = [F16._run(m, dev, images_clip, images, ids, forced, [(S, S)] * 2, [(S, S)] * 2) for m in (m1, m2)]
    assert torch.equal(outs[0][0], outs[1][0])
    for a, b in zip(outs[0][1] + outs[0][2], outs[1][1] + outs[1][2]):
        assert torch.equal(a, b)
