"""NF4 fine-tuning (QLoRA) on the MI355X: haff_nf4_dequant_t_f16 bit for bit against the transpose of the CPU restatement
(tests/nf4_ref.py); LisaTrainable(dtype=float16, load_in_4bit=True) bit for bit against the fp16 trainer on the dequantised weights
(losses, every gradient, the validation outputs), against the oracle, one adapted layer at 7B / 13B width, its footprint, the
loss-scaled loop and train_ds.py --load_in_4bit with checkpoint, resume and merge.

Why zero tolerance against the fp16 trainer: the NF4 mode only moves data. Its frozen products are the fp16 trainer's kernels on
f16 values that are, element for element, the ones quant.round_trip gives the fp16 trainer as resident weights; nothing else differs."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)   # tests/nf4_ref.py and the sibling test modules
import nf4_ref as R   # noqa: E402

ALL7 = "q_proj,k_proj,v_proj,o_proj,gate_proj,up_proj,down_proj"
GEOMS = {"7b": (4096, 32, 11008), "13b": (5120, 40, 13824)}   # hidden, heads, ffn
POISON = 7.0


def _bits(t):
    return t.contiguous().view(torch.int16)


def _same(a, b):
    return (a.shape == b.shape and a.dtype == b.dtype
            and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8)))


# ---- 1. the kernel through the C ABI ---------------------------------------------------------------------------------------------
def _dequant_t_abi(dev, packed, absmax, row_map, extra_rows=3, extra_cols=16):
    """haff_nf4_dequant_t_f16 into the top-left corner of a larger poisoned buffer -> (the whole buffer, Np)"""
    import haff  # noqa: F401
    from haff.lib import load_library
    lib = load_library()
    N, K = packed.shape[0], packed.shape[1] * 2
    Np = (N + 7) // 8 * 8
    ldo = Np + extra_cols
    buf = torch.full((K + extra_rows, ldo), POISON, dtype=torch.float16, device=dev)
    p, a = packed.to(dev).contiguous(), absmax.to(dev).contiguous()
    m = None if row_map is None else row_map.to(dev, torch.int32).contiguous()
    rc = lib.haff_nf4_dequant_t_f16(p.data_ptr(), a.data_ptr(), N, K, None if m is None else m.data_ptr(), buf.data_ptr(), ldo, None)
    torch.cuda.synchronize()
    assert rc == 0
    return buf.cpu(), Np


def _check_dequant_t(dev, packed, absmax, row_map, what):
    N, K = packed.shape[0], packed.shape[1] * 2
    ref = R.dequant(packed, absmax)                          # f16 [N, K]
    want = torch.zeros((K, N), dtype=torch.float16)
    cols = torch.arange(N) if row_map is None else row_map.long()
    want[:, cols] = ref.t()
    got, Np = _dequant_t_abi(dev, packed, absmax, row_map)
    assert torch.equal(_bits(got[:K, :N]), _bits(want)), what
    assert (got[:K, N:Np] == 0).all(), f"{what}: pad columns"
    assert (got[:K, Np:] == POISON).all() and (got[K:] == POISON).all(), f"{what}: wrote outside [K][roundup(N, 8)]"


def _swiglu_map(F):
    from haff import quant
    g, u = quant.swiglu_rows(F)
    return torch.cat([g, u])


@pytest.mark.parametrize("dq", [True, False])
@pytest.mark.parametrize("N,K", [(1, 64), (13, 64), (37, 192), (70, 192), (130, 64), (264, 192)])
@pytest.mark.parametrize("mapped", [False, True])
def test_dequant_t_small_odd_shapes(dev, N, K, dq, mapped):
    """N not a multiple of 8 or of the 64-row tile, K = 64 and 192 (not a multiple of the 256-deep tile), codes and absmax from the
    CPU quantiser with and without double quantisation; row_map: a random permutation (the element-by-element store path)"""
    g = torch.Generator().manual_seed(N * 1000 + K + dq)
    w = (torch.randn((N, K), generator=g) * 0.05).half()
    w[N // 2, :64] = 0                                       # an all-zero block: absmax 0, codes 7
    packed, absmax, _ = R.quantize(w, double_quant=dq)
    row_map = torch.randperm(N, generator=g) if mapped else None
    _check_dequant_t(dev, packed, absmax, row_map, f"N{N} K{K} dq{dq} mapped{mapped}")


@pytest.mark.parametrize("which,N,K", [("rope", 768, 64), ("rope", 1536, 192), ("swiglu", 96, 192), ("swiglu", 160, 64), ("swiglu", 352, 64)])
def test_dequant_t_model_row_maps(dev, which, N, K):
    """the maps the inference mode uses: quant.rope_row_map (q|k|v) and the [gate x16 | up x16] interleave of quant.swiglu_rows;
    both keep 8-row chunks whole, so this is the 16-byte store path under a map"""
    import haff  # noqa: F401
    from haff import quant
    g = torch.Generator().manual_seed(N + K)
    w = (torch.randn((N, K), generator=g) * 0.05).half()
    packed, absmax, _ = R.quantize(w)
    row_map = quant.rope_row_map(N, "cpu").long() if which == "rope" else _swiglu_map(N // 2)
    assert sorted(row_map.tolist()) == list(range(N))
    _check_dequant_t(dev, packed, absmax, row_map, f"{which} N{N} K{K}")


@pytest.mark.parametrize("geom", ["7b", "13b"])
@pytest.mark.parametrize("proj", ["qkv", "o", "gate_up", "down"])
def test_dequant_t_projection_shapes(dev, geom, proj):
    """the four projection shapes at 7B and 13B width on random codes and absmax (every code, absmax over six decades), without a
    map and, for q|k|v and gate|up, with theirs; Nf4Weight.dequant_t against Nf4Weight.dequant on the device as well"""
    import haff  # noqa: F401
    from haff import quant
    H, _, F = GEOMS[geom]
    N, K = {"qkv": (3 * H, H), "o": (H, H), "gate_up": (2 * F, H), "down": (H, F)}[proj]
    g = torch.Generator().manual_seed(N + K)
    packed = torch.randint(0, 256, (N, K // 2), generator=g, dtype=torch.uint8)
    absmax = torch.exp(torch.rand((N, K // 64), generator=g) * 13.8 - 11.5)
    _check_dequant_t(dev, packed, absmax, None, f"{geom} {proj}")
    if proj in ("qkv", "gate_up"):
        row_map = quant.rope_row_map(N, "cpu").long() if proj == "qkv" else _swiglu_map(F)
        _check_dequant_t(dev, packed, absmax, row_map, f"{geom} {proj} mapped")
    q = quant.Nf4Weight(packed.to(dev), absmax.to(dev))
    assert torch.equal(_bits(q.dequant_t()), _bits(q.dequant().t().contiguous()))


def test_dequant_t_bad_arguments_return_minus_one_without_a_launch(dev):
    import haff  # noqa: F401
    from haff.lib import load_library
    lib = load_library()
    out = torch.full((64, 32), POISON, dtype=torch.float16, device=dev)
    packed = torch.zeros((16, 32), dtype=torch.uint8, device=dev)
    absmax = torch.ones((16, 1), dtype=torch.float32, device=dev)

    def d(N, K, ldo, p=packed.data_ptr(), a=absmax.data_ptr(), o=out.data_ptr()):
        return int(lib.haff_nf4_dequant_t_f16(p, a, N, K, None, o, ldo, None))
    assert d(16, 96, 32) == -1 and d(16, 64, 12) == -1 and d(16, 64, 8) == -1 and d(0, 64, 32) == -1
    assert d(16, 64, 32, p=packed.data_ptr() + 4) == -1 and d(16, 64, 32, o=out.data_ptr() + 8) == -1
    assert d(16, 64, 32, p=None) == -1 and d(16, 64, 32, a=None) == -1 and d(16, 64, 32, o=None) == -1
    torch.cuda.synchronize()
    assert (out == POISON).all()
    assert d(16, 64, 32) == 0
    torch.cuda.synchronize()
    assert (out[:, :16] == -1.0).all() and (out[:, 16:] == POISON).all()   # code 0 = -1.0, absmax 1


# ---- shared: weights, batches, one forward + backward ----------------------------------------------------------------------------
def _weights(cfg, dev, seed=21):
    """(sd, sd_rt): sd_rt replaces exactly the tensors the NF4 trainer quantises by quant.round_trip of themselves"""
    import haff  # noqa: F401
    from haff import quant, weights as hw
    from haff.train_model import nf4_frozen_linear
    from test_fp16_train_gpu import _exact_in_all
    sd = _exact_in_all(hw.make_state_dict(cfg, seed))
    sd_rt, n = {}, 0
    for k, v in sd.items():
        if nf4_frozen_linear(k):
            sd_rt[k] = quant.round_trip(v, dev).float().cpu()
            assert not torch.equal(sd_rt[k], v.float()), k   # quantisation moves the values: the comparison below is not vacuous
            n += 1
        else:
            sd_rt[k] = v
    assert n == 7 * cfg.llm.layers + 1
    assert cfg.llm.layers >= 2   # a stale scratch buffer (another layer's weights) cannot pass
    assert not torch.equal(sd["model.layers.0.self_attn.q_proj.weight"], sd["model.layers.1.self_attn.q_proj.weight"])
    return sd, sd_rt


def _dev_batch(cfg, dev, seed=0):
    from test_fp16_train_gpu import _batch
    return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in _batch(cfg, seed).items()}


def _step(model, batch, seed=1234):
    model.zero_grad()
    torch.manual_seed(seed)   # the dropout masks are drawn on the device: the same seed gives both trainers the same masks
    out = model(**batch)
    out["loss"].backward()
    torch.cuda.synchronize()
    return ({k: v.detach().float().cpu() for k, v in out.items()},
            {k: (None if p.grad is None else p.grad.detach().clone()) for k, p in model.named_parameters()})


def _pair(cfg, dev, sd, sd_rt, **kw):
    from haff.train_model import LisaTrainable
    m4 = LisaTrainable(cfg, sd, dtype=torch.float16, device=dev, load_in_4bit=True, **kw)
    m16 = LisaTrainable(cfg, sd_rt, dtype=torch.float16, device=dev, **kw)
    return m4, m16


# ---- 2. the trainer equals the fp16 trainer on the dequantised weights, bit for bit --------------------------------------------
@pytest.mark.parametrize("geom", ["tiny", "mid"])
@pytest.mark.parametrize("case", ["qv", "proj_fused", "all7_generic", "r0"])
def test_nf4_trainer_bitwise_equals_fp16_trainer_on_dequantised_weights(dev, geom, case):
    import haff  # noqa: F401
    from haff import autograd as A
    from haff import config as hcfg
    cfg = getattr(hcfg, geom)()
    sd, sd_rt = _weights(cfg, dev)
    batch = _dev_batch(cfg, dev)
    targets, fused, r = {"qv": ("q_proj,v_proj", True, 8), "proj_fused": ("proj", True, 8), "all7_generic": (ALL7, False, 8),
                         "r0": ("q_proj,v_proj", True, 0)}[case]
    m4, m16 = _pair(cfg, dev, sd, sd_rt, lora_r=r, lora_dropout=0.05, lora_init_b_zero=False, seed=3, lora_target_modules=targets)
    assert len(m4.lora_modules) == {"qv": 2, "proj_fused": 7, "all7_generic": 7, "r0": 0}[case] * cfg.llm.layers
    assert m4.training and m4.lora_dropout == 0.05
    try:
        A.FUSED_LORA_QKV = A.FUSED_LORA_OUT = A.FUSED_LORA_GATE_UP = fused
        l4, g4 = _step(m4, batch)
        l16, g16 = _step(m16, batch)
        l4b, g4b = _step(m4, batch)   # a second step of the NF4 trainer, compared below
    finally:
        A.FUSED_LORA_QKV = A.FUSED_LORA_OUT = A.FUSED_LORA_GATE_UP = True
    assert set(l4) == {"loss", "ce_loss", "taxonomy_ce_loss", "mask_bce_loss", "mask_dice_loss", "mask_loss"}
    for k in l4:
        print(f"{geom} {case} {k}: nf4 {float(l4[k]):.8f} fp16 on dequantised weights {float(l16[k]):.8f}")
        assert torch.isfinite(l4[k]).all() and _same(l4[k], l16[k]), k
    assert list(g4) == list(g16)
    n = 0
    for k in g4:
        assert (g4[k] is None) == (g16[k] is None), k
        if g4[k] is not None:
            assert torch.isfinite(g4[k].float()).all(), k
            assert _same(g4[k], g16[k]), f"{geom} {case}: gradient of {k} differs"
            n += 1
    lora = [k for k in g4 if "lora_" in k]
    assert len(lora) == 2 * len(m4.lora_modules) and all(g4[k] is not None and g4[k].abs().max() > 0 for k in lora)
    assert n > 100
    # a second step on the NF4 trainer gives the same bits again (the scratch buffers carry nothing over)
    assert all(_same(l4[k], l4b[k]) for k in l4) and all(g4[k] is None or _same(g4[k], g4b[k]) for k in g4)


# ---- 3. against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["tiny", "mid"])
def test_nf4_trainer_matches_oracle_on_dequantised_weights(dev, geom):
    """the oracle's model_forward under autograd on sd_rt, with the fp16 trainer's bounds (tests/test_fp16_train_gpu.py: losses
    3e-2, every tensor 0.25, per class BF16_CLASS_TOL)"""
    import haff  # noqa: F401
    from haff import config as hcfg
    from haff.train_model import LisaTrainable
    from oracle import lisa_oracle as O
    from test_fp16_train_gpu import BF16_CLASS_TOL, _batch, _class
    cfg = getattr(hcfg, geom)()
    sd, sd_rt = _weights(cfg, dev)
    batch = _batch(cfg)
    model = LisaTrainable(cfg, sd, dtype=torch.float16, device=dev, lora_dropout=0.0, lora_init_b_zero=False, seed=3, load_in_4bit=True)
    osd = {k: v.clone() for k, v in sd_rt.items()}
    lora = {}
    for k, p in model.named_parameters():
        t = p.detach().float().cpu().clone().requires_grad_(True)
        (lora if "lora_" in k else osd)[k] = t
    ref = O.lisa_model_forward(osd, cfg, batch, lora=lora)
    ref["loss"].backward()
    out = model(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()})
    out["loss"].backward()
    for k in ref:
        a, b = float(out[k]), float(ref[k])
        print(f"nf4 {geom} {k}: hip {a:.6f} oracle {b:.6f}")
        assert abs(a - b) <= 3e-2 * max(1.0, abs(b)), k
    by, n = {}, 0
    for k, p in model.named_parameters():
        r = (lora[k] if "lora_" in k else osd[k]).grad
        if r is None or p.grad is None or r.abs().max().item() < 1e-6:
            continue
        v = ((p.grad.float().cpu() - r).norm() / (r.norm() + 1e-12)).item()
        assert v <= 0.25, (k, v)
        by[_class(k)] = max(by.get(_class(k), 0.0), v)
        n += 1
    print("nf4 per class worst relative L2: " + ", ".join(f"{c} {by[c]:.3e}" for c in sorted(by)))
    assert n > 100
    for c, v in by.items():
        assert v <= BF16_CLASS_TOL.get(c, 0.25), (c, v)


# ---- 4. one adapted layer at 7B / 13B width --------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["7b", "13b"])
def test_nf4_adapted_layers_at_full_width_bitwise(dev, geom):
    """Two Llama layers with different weights at 7B / 13B width, all seven adapters on the fused nodes with per-adapter masks,
    351 tokens: A.Nf4FrozenWeight (codes + shared scratch) against the same nodes on resident round-tripped weights, forward and
    every gradient, bit for bit. The second layer overwrites the scratch before the first layer's backward runs."""
    import haff  # noqa: F401
    from haff import autograd as A
    from haff import quant
    H, heads, F = GEOMS[geom]
    T, r, s = 351, 8, 2.0 / 0.95
    g = torch.Generator(device=dev).manual_seed(77 + H)

    def rn(shape, scale=1.0):
        return (torch.randn(shape, generator=g, device=dev) * scale).half()
    shapes = {"wqkv": (3 * H, H), "wo": (H, H), "wgu": (2 * F, H), "wd": (H, F)}
    scratch = {}
    for (N, K) in shapes.values():
        scratch["w", (N, K)] = torch.empty((N, K), dtype=torch.float16, device=dev)
        scratch["w_t", (N, K)] = torch.empty((K, N), dtype=torch.float16, device=dev)
    nf4, res = [], []
    for _ in range(2):
        qs = {n: quant.quantize([(rn(sh, sh[1] ** -0.5), None)], dev) for n, sh in shapes.items()}
        nf4.append({n: A.Nf4FrozenWeight(q, scratch) for n, q in qs.items()})
        res.append({n: A.FrozenWeight(q.dequant(), A.transpose(q.dequant())[0]) for n, q in qs.items()})
    theta = torch.rand((T, 64), generator=g, device=dev) * 6.0
    cs = torch.cat([theta.cos(), theta.sin()], 1).contiguous()
    dims = {"q": (H, H), "v": (H, H), "k": (H, H), "o": (H, H), "g": (H, F), "u": (H, F), "d": (F, H)}   # (in, out)
    leaves0 = [rn((T, H))]
    for _ in range(2):
        for fin, fout in dims.values():
            leaves0 += [rn((r, fin), fin ** -0.5), rn((fout, r), 0.05)]
    keeps = [[(torch.rand((T, fin), generator=g, device=dev) >= 0.3).half() for fin, _ in dims.values()] for _ in range(2)]
    dy = rn((T, H), 0.1)
    gain = torch.ones((H,), dtype=torch.float32, device=dev)   # pre-norm layers, as LisaTrainable._llm builds them

    def run(W):
        leaves = [t.detach().clone().requires_grad_(True) for t in leaves0]
        x = leaves[0]
        for li in range(2):
            p = leaves[1 + 14 * li: 15 + 14 * li]
            (aq, bq), (av, bv), (ak, bk), (ao, bo), (ag, bg), (au, bu), (ad, bd) = [(p[2 * i], p[2 * i + 1]) for i in range(7)]
            kq, kv, kk, ko, kg, ku, kd = keeps[li]
            h = A.rmsnorm(x, gain, 1e-6)
            q, k, v = A.lora_qkv3_rope(h, W[li]["wqkv"], None, aq, bq, av, bv, ak, bk, cs, T, heads, s, (kq, kv, kk))
            a = A.attention(q.view(1, T, H), k.view(1, T, H), v.view(1, T, H), heads, 128 ** -0.5, True)
            x = A.lora_linear(a.view(T, H), W[li]["wo"], None, x, ao, bo, s, ko)
            y = A.lora_gate_up_swiglu(A.rmsnorm(x, gain, 1e-6), W[li]["wgu"], None, ag, bg, au, bu, s, (kg, ku))
            x = A.lora_linear(y, W[li]["wd"], None, x, ad, bd, s, kd)
        x.backward(dy)
        torch.cuda.synchronize()
        return x.detach(), [t.grad for t in leaves]
    y4, g4 = run(nf4)
    y16, g16 = run(res)
    print(f"{geom}: |y| max {y4.float().abs().max().item():.3f}; leaves finite nf4 / resident: "
          + " ".join(f"{int(torch.isfinite(a.float()).all())}{int(torch.isfinite(b.float()).all())}" for a, b in zip(g4, g16)))
    assert torch.isfinite(y4.float()).all() and _same(y4, y16)
    for i, (a, b) in enumerate(zip(g4, g16)):
        assert a is not None and torch.isfinite(a.float()).all() and a.abs().max() > 0, i
        assert _same(a, b), f"{geom}: gradient of leaf {i} differs"


# ---- 5. footprint ------------------------------------------------------------------------------------------------------------
def _peak_over_one_step(model, batch):
    import gc
    gc.collect()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    _step(model, batch)
    return torch.cuda.max_memory_allocated()


def test_nf4_trainer_footprint(dev):
    import gc
    import haff  # noqa: F401
    from haff import config as hcfg, quant
    from haff.train_model import LisaTrainable
    cfg = hcfg.mid()
    sd, sd_rt = _weights(cfg, dev)
    batch = _dev_batch(cfg, dev)
    kw = dict(lora_dropout=0.05, lora_init_b_zero=False, seed=3, lora_target_modules=ALL7)
    model = LisaTrainable(cfg, sd, dtype=torch.float16, device=dev, load_in_4bit=True, **kw)
    peak4 = _peak_over_one_step(model, batch)
    assert not model.wt                                     # no resident W^T
    names = ("wqkv", "wo", "wgu", "wd")
    seen, expect = {}, 0
    for L, Fz in zip(model.base.llm.layers, model.frozen):
        for n in names:
            assert isinstance(L[n], quant.Nf4Weight) and Fz[n].q is L[n]
            expect += L[n].nbytes
            for obj in (L[n], Fz[n]):                       # every tensor a frozen projection holds on to
                for v in vars(obj).values():
                    for t in (v.values() if isinstance(v, dict) else [v]):
                        if torch.is_tensor(t):
                            seen[t.data_ptr()] = t.numel() * t.element_size()
    scratch = sum(t.numel() * t.element_size() for t in model.nf4_scratch.values())
    H, F = cfg.llm.hidden, cfg.llm.ffn
    assert scratch == 2 * 2 * (3 * H * H + H * H + 2 * F * H + H * F)   # one [N, K] and one [K, N] f16 buffer per projection shape
    assert sum(seen.values()) == expect + scratch
    assert expect * 16 == cfg.llm.layers * (3 * H * H + H * H + 2 * F * H + H * F) * 9   # 4.5 bits per weight
    assert model.base.fc0 is None and model.base.fc2 is None and isinstance(model.base.llm.lm_head, torch.Tensor)
    del model, seen
    gc.collect()
    model = LisaTrainable(cfg, sd_rt, dtype=torch.float16, device=dev, **kw)
    peak16 = _peak_over_one_step(model, batch)
    print(f"peak bytes over one step at mid geometry: nf4 {peak4} fp16 {peak16}")
    assert peak4 < peak16


# ---- 6. loop and files -----------------------------------------------------------------------------------------------------------
def _loop(dev, steps=6, seed=22, base_lr=3e-4):
    """tests/test_fp16_train_gpu.py::_loop (same seeds, learning rate and scaler) on the NF4 base"""
    from haff import config as hcfg, weights as hw
    from haff import train_ops as T
    from haff.train_model import LisaTrainable
    from test_fp16_train_gpu import _exact_in_all
    from test_train_gpu import make_batch
    cfg = hcfg.tiny()
    sd = _exact_in_all(hw.make_state_dict(cfg, seed))
    model = LisaTrainable(cfg, sd, dtype=torch.float16, device=dev, lora_dropout=0.0, lora_init_b_zero=False, load_in_4bit=True)
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in make_batch(cfg, seed=1).items()}
    named = model.named_parameters()
    reducer = T.GradBucketReducer(named)
    opt = T.BucketAdamW(reducer, named)
    scaler = T.DynamicLossScaler(init_scale=2.0 ** 16)
    rec, taken = [], 0
    for _ in range(steps):
        reducer.zero()
        reducer.begin(sync=True)
        out = model(**batch)
        (out["loss"] * scaler.loss_scale).backward()
        reducer.finish()
        gscale = 1.0 / scaler.loss_scale
        norm = T.grad_norm(reducer.grads())
        lr = T.warmup_decay_lr(taken, 100, base_lr, warmup_steps=0)
        opt.step(lr=lr, gscale=gscale, gscale_dev=T.clip_coef_device(norm * gscale, 1.0), skip_norm=norm)
        scale_used = scaler.loss_scale
        skipped = scaler.update_scale(not bool(torch.isfinite(norm).item()))
        if skipped:
            opt.unstep()
        else:
            taken += 1
        rec.append((float(out["loss"]), scale_used, skipped, opt.step_count))
    return rec, model


def test_nf4_loop_with_loss_scaling_lowers_the_loss_and_repeats_bitwise(dev):
    import haff  # noqa: F401
    rec, m1 = _loop(dev)
    print(rec)
    taken = [r for r in rec if not r[2]]
    assert len(taken) >= 4 and rec[-1][0] < rec[0][0]
    rec2, m2 = _loop(dev)
    assert rec == rec2
    for (k, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(a, b), k


def test_train_ds_load_in_4bit_cli_checkpoint_resume_and_merge(dev, tmp_path, capsys):
    import haff  # noqa: F401
    from haff import checkpoint, config as hcfg, merge_lora, train_ds
    from haff.lisa import LisaMI355
    common = ["--synthetic", "tiny", "--grad_accumulation_steps", "1", "--batch_size", "2", "--mask_hw", "64", "48", "--lora_dropout", "0",
              "--no_eval", "--lr", "0.0003", "--precision", "fp16", "--print_freq", "1", "--log_base_dir", str(tmp_path), "--exp_name", "q"]
    train_ds.main(common + ["--load_in_4bit", "--epochs", "1", "--steps_per_epoch", "2"])
    out = capsys.readouterr().out
    assert "LossScale" in out and "Epoch: [0][2/2]" in out and "saved checkpoint" in out
    path = tmp_path / "q" / "ckpt_model" / "latest.pt"
    blob = torch.load(path, map_location="cpu", weights_only=False)
    assert blob["base_format"] == "nf4" and blob["global_step"] == 2
    # trainable-only: no packed codes, no frozen projection
    assert all(v.dtype in (torch.float16, torch.float32) for v in blob["params"].values())
    assert not any(k.endswith("_proj.weight") and k.startswith("model.layers.") for k in blob["params"])
    train_ds.main(common + ["--load_in_4bit", "--epochs", "2", "--steps_per_epoch", "2"])
    out = capsys.readouterr().out
    assert "resume training from" in out and "Epoch: [1][2/2]" in out
    assert torch.load(path, map_location="cpu", weights_only=False)["global_step"] == 4
    with pytest.raises(ValueError, match=r"NF4 \(--load_in_4bit\) base.*pass --load_in_4bit"):
        train_ds.main(common + ["--epochs", "3", "--steps_per_epoch", "2"])
    capsys.readouterr()
    # a checkpoint from before the field existed resumes as the 16-bit base, and is refused under --load_in_4bit by name
    train_ds.main(common[:-1] + ["old", "--epochs", "1", "--steps_per_epoch", "1"])
    old = tmp_path / "old" / "ckpt_model" / "latest.pt"
    b = torch.load(old, map_location="cpu", weights_only=False)
    assert b["base_format"] is None
    del b["base_format"]
    torch.save(b, old)
    capsys.readouterr()
    train_ds.main(common[:-1] + ["old", "--epochs", "2", "--steps_per_epoch", "1"])
    assert "resume training from" in capsys.readouterr().out
    with pytest.raises(ValueError, match=r"16-bit base.*drop --load_in_4bit"):
        train_ds.main(common[:-1] + ["old", "--load_in_4bit", "--epochs", "3", "--steps_per_epoch", "1"])
    capsys.readouterr()
    # merge into the ORIGINAL 16-bit weights; the result is served with load_in_4bit=True
    blob = torch.load(path, map_location="cpu", weights_only=False)
    cfg = hcfg.tiny()
    sd = checkpoint.synthetic_state_dict(cfg, 1234, dev, torch.float16)
    merged = merge_lora.merge_state_dict(sd, blob["params"], 8, 16, torch.float16)
    qk = "model.layers.0.self_attn.q_proj.weight"
    a, b_ = blob["params"][qk[:-7] + ".lora_A"].float(), blob["params"][qk[:-7] + ".lora_B"].float()
    assert torch.equal(merged[qk], (sd[qk].float().cpu() + 2.0 * (b_ @ a)).half())
    merged.update({k: v for k, v in sd.items() if k not in merged})
    m = LisaMI355(cfg, merged, dtype=torch.float16, device=dev, load_in_4bit=True)
    assert m.load_in_4bit
    # merge_lora's CLI prints the reminder for such a checkpoint
    from haff import merge_lora as ML
    vdir = tmp_path / "base"
    ML.save_pretrained(OrderedDictCPU(sd), str(vdir), ML.hf_config(cfg, torch.float16))
    ML.main(["--version", str(vdir), "--weight", str(path), "--save_path", str(tmp_path / "merged"), "--precision", "fp16"])
    out = capsys.readouterr().out
    assert "trained on the NF4 base" in out and "load_in_4bit=True" in out and "merged 4 LoRA pairs" in out


def OrderedDictCPU(sd):
    from collections import OrderedDict
    return OrderedDict((k, v.detach().cpu().contiguous()) for k, v in sd.items() if "vision_tower" not in k)


# ---- 7. validation path ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", ["tiny", "mid"])
def test_nf4_validation_forward_bitwise_equals_fp16_trainer(dev, geom):
    import haff  # noqa: F401
    from haff import config as hcfg
    cfg = getattr(hcfg, geom)()
    sd, sd_rt = _weights(cfg, dev)
    batch = _dev_batch(cfg, dev, 2)
    m4, m16 = _pair(cfg, dev, sd, sd_rt, lora_init_b_zero=False, seed=3, lora_target_modules=ALL7)
    outs = []
    for m in (m4, m16):
        m.eval()
        with torch.no_grad():
            outs.append(m(**{**batch, "inference": True}))
    a, b = outs
    assert set(a) == {"pred_masks_left", "pred_masks_right", "pred_taxonomies", "gt_masks_left", "gt_masks_right", "gt_taxonomies"}
    for k in a:
        assert torch.isfinite(a[k].float()).all() and _same(a[k], b[k]), k
    assert a["pred_masks_left"].abs().max() > 0
