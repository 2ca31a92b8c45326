"""LoRA on every Llama projection on the MI355X: the fused adapter nodes (csrc/lora.hip: q|k|v with three adapters, o / down with
haff_lora_out, gate|up with haff_lora_gu_swiglu) against torch fp32 compositions of the same arithmetic, the all-seven trainer
against the oracle (every adapter merged into its weight by the test), fused against generic, repeatability, dropout masks,
merge, and train_ds --lora_target_modules / --lora_r 0 with checkpoint and resume."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ALL7 = "q_proj,k_proj,v_proj,o_proj,gate_proj,up_proj,down_proj"
DTYPES = [torch.bfloat16, torch.float16]


def _rand(shape, g, scale=1.0):
    return (torch.randn(shape, generator=g) * scale)


def _masks(n, shape, g, p=0.3):
    return [(torch.rand(shape, generator=g) >= p).float() for _ in range(n)]


def _close(got, ref, tol, what):
    err = (got.float().cpu() - ref).abs().max().item() / (ref.abs().max().item() + 1e-12)
    print(f"{what}: rel {err:.3e}")
    assert err <= tol, (what, err)


def _leaf(t, dev, dtype):
    return t.to(dev, dtype).requires_grad_(True), t.to(dtype).float().requires_grad_(True)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("masked", [False, True])
def test_lora_linear_node(dev, dtype, masked):
    """y = x W^T + resid + s ((x o keep) A^T) B^T (haff_lora_out) and its adjoint, M = 50, K = 512 (down) / 256 (o)."""
    import haff  # noqa: F401
    from haff import autograd as A
    g = torch.Generator().manual_seed(1)
    for M, K, N, r in ((50, 512, 256, 8), (37, 256, 256, 5)):
        x32, w32, res32 = _rand((M, K), g), _rand((N, K), g, K ** -0.5), _rand((M, N), g)
        a32, b32 = _rand((r, K), g, K ** -0.5), _rand((N, r), g, 0.1)
        keep = _masks(1, (M, K), g)[0] if masked else None
        s = 2.0 / 0.7
        x, xr = _leaf(x32, dev, dtype)
        res, resr = _leaf(res32, dev, dtype)
        a, ar = _leaf(a32, dev, dtype)
        b, br = _leaf(b32, dev, dtype)
        w = w32.to(dev, dtype)
        wr = w32.to(dtype).float()
        y = A.lora_linear(x, w, A.transpose(w)[0], res, a, b, s, None if keep is None else keep.to(dev, dtype))
        xd = xr if keep is None else xr * keep
        yr = xr @ wr.t() + resr + s * (xd @ ar.t()) @ br.t()
        dy = _rand((M, N), g)
        y.backward(dy.to(dev, dtype))
        yr.backward(dy.to(dtype).float())
        tol = 2e-2 if dtype == torch.bfloat16 else 4e-3
        _close(y, yr.detach(), tol, f"{dtype} M{M} K{K} y")
        for n, t, tr in (("dx", x, xr), ("dresid", res, resr), ("dA", a, ar), ("dB", b, br)):
            _close(t.grad, tr.grad, tol, f"{dtype} M{M} K{K} {n}")


def _interleave(gate, up):
    M, F = gate.shape
    return torch.cat([gate.view(M, F // 16, 1, 16), up.view(M, F // 16, 1, 16)], 2).reshape(M, 2 * F)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("masks", [0, 1, 2])
def test_lora_gate_up_swiglu_node(dev, dtype, masks):
    """gu' = x Wgu^T + both rank updates in the interleaved layout (haff_lora_gu_swiglu), y = silu(g') u', and the adjoint."""
    import haff  # noqa: F401
    from haff import autograd as A
    g = torch.Generator().manual_seed(2)
    M, K, F, r = 45, 256, 512, 8
    x32, a_g, a_u = _rand((M, K), g), _rand((r, K), g, K ** -0.5), _rand((r, K), g, K ** -0.5)
    w32 = _rand((2 * F, K), g, K ** -0.5)
    b_g, b_u = _rand((F, r), g, 0.2), _rand((F, r), g, 0.2)
    ks = _masks(2, (M, K), g)
    keep = None if masks == 0 else (ks[0] if masks == 1 else tuple(ks))
    s = 2.0
    x, xr = _leaf(x32, dev, dtype)
    ag, agr = _leaf(a_g, dev, dtype)
    au, aur = _leaf(a_u, dev, dtype)
    bg, bgr = _leaf(b_g, dev, dtype)
    bu, bur = _leaf(b_u, dev, dtype)
    w = w32.to(dev, dtype)
    wr = w32.to(dtype).float()
    kd = None if keep is None else (keep.to(dev, dtype) if masks == 1 else tuple(k.to(dev, dtype) for k in keep))
    y = A.lora_gate_up_swiglu(x, w, A.transpose(w)[0], ag, bg, au, bu, s, kd)
    kg = 1.0 if masks == 0 else (ks[0])
    ku = 1.0 if masks == 0 else (ks[0] if masks == 1 else ks[1])
    gu = xr @ wr.t() + _interleave(s * ((xr * kg) @ agr.t()) @ bgr.t(), s * ((xr * ku) @ aur.t()) @ bur.t())
    gate, up = gu.view(M, F // 16, 2, 16)[:, :, 0].reshape(M, F), gu.view(M, F // 16, 2, 16)[:, :, 1].reshape(M, F)
    yr = torch.nn.functional.silu(gate) * up
    dy = _rand((M, F), g)
    y.backward(dy.to(dev, dtype))
    yr.backward(dy.to(dtype).float())
    tol = 3e-2 if dtype == torch.bfloat16 else 5e-3
    _close(y, yr.detach(), tol, f"{dtype} y")
    for n, t, tr in (("dx", x, xr), ("dAg", ag, agr), ("dAu", au, aur), ("dBg", bg, bgr), ("dBu", bu, bur)):
        _close(t.grad, tr.grad, tol, f"{dtype} masks {masks} {n}")


def _rope_ref(q, cs, T):
    pos = torch.arange(q.shape[0]) % T
    co, si = cs[pos, :64].repeat(1, q.shape[1] // 128), cs[pos, 64:].repeat(1, q.shape[1] // 128)
    qh = q.view(q.shape[0], -1, 2, 64)
    lo, hi = qh[:, :, 0].reshape(q.shape[0], -1), qh[:, :, 1].reshape(q.shape[0], -1)
    o1, o2 = lo * co - hi * si, hi * co + lo * si
    return torch.stack([o1.view(q.shape[0], -1, 64), o2.view(q.shape[0], -1, 64)], 2).reshape(q.shape)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["qkv_none", "qkv_one", "qkv_three", "k_only"])
def test_lora_qkv3_rope_node(dev, dtype, case):
    """The three-adapter q|k|v + RoPE node (haff_lora_qkv3_rope_fwd, haff_lora_dx3) against torch fp32, M = 50."""
    import haff  # noqa: F401
    from haff import autograd as A
    g = torch.Generator().manual_seed(3)
    M, T, H, r = 50, 25, 256, 8
    theta = torch.rand((T, 64), generator=g) * 6.0
    cs = torch.cat([theta.cos(), theta.sin()], 1)
    x32, w32 = _rand((M, H), g), _rand((3 * H, H), g, H ** -0.5)
    ad = [_rand((r, H), g, H ** -0.5) for _ in range(3)]      # q, v, k
    bd = [_rand((H, r), g, 0.2) for _ in range(3)]
    on = [True, True, True] if case != "k_only" else [False, False, True]
    ks = _masks(3, (M, H), g)
    keep = {"qkv_none": None, "qkv_one": ks[0], "qkv_three": tuple(ks), "k_only": tuple(ks)}[case]
    s = 2.0
    x, xr = _leaf(x32, dev, dtype)
    leaves = [(_leaf(ad[i], dev, dtype), _leaf(bd[i], dev, dtype)) if on[i] else ((None, None), (None, None)) for i in range(3)]
    w = w32.to(dev, dtype)
    wr = w32.to(dtype).float()
    kd = None if keep is None else (keep.to(dev, dtype) if torch.is_tensor(keep) else tuple(k.to(dev, dtype) for k in keep))
    (aq, _), (bq, _) = leaves[0]
    (av, _), (bv, _) = leaves[1]
    (ak, _), (bk, _) = leaves[2]
    q, k, v = A.lora_qkv3_rope(x, w, A.transpose(w)[0], aq, bq, av, bv, ak, bk, cs.to(dev), T, H // 128, s, kd)
    qkv = xr @ wr.t()
    outs = [qkv[:, :H], qkv[:, 2 * H:], qkv[:, H:2 * H]]
    for i in range(3):
        if on[i]:
            km = 1.0 if keep is None else (keep if torch.is_tensor(keep) else keep[i])
            outs[i] = outs[i] + s * ((xr * km) @ leaves[i][0][1].t()) @ leaves[i][1][1].t()
    qr, vr, kr = _rope_ref(outs[0], cs, T), outs[1], _rope_ref(outs[2], cs, T)
    dq, dk, dv = _rand((M, H), g), _rand((M, H), g), _rand((M, H), g)
    torch.autograd.backward([q, k, v], [t.to(dev, dtype) for t in (dq, dk, dv)])
    torch.autograd.backward([qr, kr, vr], [t.to(dtype).float() for t in (dq, dk, dv)])
    tol = 2e-2 if dtype == torch.bfloat16 else 4e-3
    for n, a_, b_ in (("q", q, qr), ("k", k, kr), ("v", v, vr)):
        _close(a_, b_.detach(), tol, f"{dtype} {case} {n}")
    _close(x.grad, xr.grad, tol, f"{dtype} {case} dx")
    for i, n in enumerate("qvk"):
        if on[i]:
            _close(leaves[i][0][0].grad, leaves[i][0][1].grad, tol, f"{dtype} {case} dA{n}")
            _close(leaves[i][1][0].grad, leaves[i][1][1].grad, tol, f"{dtype} {case} dB{n}")


# ---- the trainer -------------------------------------------------------------------------------------------------------------
def _batch(cfg):
    sys.path.insert(0, HERE)
    from test_train_gpu import make_batch
    return make_batch(cfg)


def _class(key):
    sys.path.insert(0, HERE)
    from test_train_gpu import grad_class
    return grad_class(key)


BF16_CLASS_TOL = {"lora_A": 3e-2, "lora_B": 3e-2, "embed_tokens": 2e-2, "lm_head": 1.2e-2, "text_hidden_fcs": 0.2,
                  "decoder.output_upscaling": 3e-2}   # the bf16 test's per-class bounds (tests/test_train_gpu.py)
# the mid geometry (256-wide mask decoder): decoder.output_upscaling measured 7.06e-2 in bf16 on MI355X with all seven targets
# (the adapter classes there: lora_A 1.75e-2, lora_B 1.59e-2); the bound is 2x that measurement, as test_train_gpu.py's are
MID_CLASS_TOL = {**BF16_CLASS_TOL, "decoder.output_upscaling": 0.15}


def _merged_oracle(cfg, sd, model, batch, alpha=16.0):
    """oracle.lisa_model_forward on weights W + (alpha / r) B A of EVERY adapter (leaf tensors with requires_grad)."""
    from oracle import lisa_oracle as O
    osd = {k: v.clone() for k, v in sd.items()}
    lora, other = {}, {}
    for k, p in model.named_parameters():
        t = p.detach().float().cpu().clone().requires_grad_(True)
        (lora if "lora_" in k else other)[k] = t
    osd.update(other)
    for k in [k for k in lora if k.endswith(".lora_A")]:
        mod = k[:-len(".lora_A")]
        a, b = lora[k], lora[mod + ".lora_B"]
        osd[mod + ".weight"] = sd[mod + ".weight"] + (alpha / a.shape[0]) * (b @ a)
    ref = O.lisa_model_forward(osd, cfg, batch, lora=None)
    ref["loss"].backward()
    return ref, {**lora, **other}


@pytest.mark.parametrize("geom", ["tiny", "mid"])
@pytest.mark.parametrize("mode", ["f32", "bf16", "fp16"])
def test_all_seven_trainer_matches_oracle(dev, geom, mode):
    import haff  # noqa: F401
    from haff import config as hcfg, weights as hw
    from haff.train_model import LisaTrainable
    cfg = getattr(hcfg, geom)()
    sd = hw.make_state_dict(cfg, 21)
    batch = _batch(cfg)
    if mode != "f32":
        hw.round_to_bf16_(sd)
        batch["images"] = batch["images"].to(torch.bfloat16).float()
        batch["images_clip"] = batch["images_clip"].to(torch.bfloat16).float()
    dtype = {"f32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[mode]
    model = LisaTrainable(cfg, sd, dtype=dtype, device=dev, lora_dropout=0.0, lora_init_b_zero=False, seed=3,
                          lora_target_modules=ALL7)
    assert len(model.lora_modules) == 7 * cfg.llm.layers
    ref, leaves = _merged_oracle(cfg, sd, model, batch)
    out = model(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()})
    out["loss"].backward()
    ltol = 1e-4 if mode == "f32" else 3e-2
    for k in ref:
        a, b = float(out[k].detach()), float(ref[k].detach())
        print(f"{geom} {mode} {k}: hip {a:.6f} oracle {b:.6f}")
        assert abs(a - b) <= ltol * max(1.0, abs(b)), k
    by_class, fg, fr, n = {}, [], [], 0
    for k, p in model.named_parameters():
        r = leaves[k].grad
        if r is None or r.abs().max().item() < 1e-6:
            continue
        assert p.grad is not None, k
        if mode == "f32":
            rel = (p.grad.float().cpu() - r).abs().max().item() / r.abs().max().item()
            assert rel <= 2e-3, (k, rel)
        else:
            rel = ((p.grad.float().cpu() - r).norm() / (r.norm() + 1e-12)).item()
            assert rel <= 0.25, (k, rel)
        by_class[_class(k)] = max(by_class.get(_class(k), 0.0), rel)
        fg.append(p.grad.float().cpu().reshape(-1))
        fr.append(r.reshape(-1))
        n += 1
    print(f"{geom} {mode}: {n} gradients; worst per class " + ", ".join(f"{c} {v:.3e}" for c, v in sorted(by_class.items())))
    assert sum(1 for k in model.params if "lora_" in k and leaves[k].grad is not None) == 14 * cfg.llm.layers
    if mode != "f32":
        tol = MID_CLASS_TOL if geom == "mid" else BF16_CLASS_TOL
        for c, v in by_class.items():
            assert v <= tol.get(c, 0.25), (c, v)
    cos = torch.nn.functional.cosine_similarity(torch.cat(fg).double(), torch.cat(fr).double(), dim=0).item()
    print(f"{geom} {mode}: global gradient cosine {cos:.6f}")
    assert cos >= (0.99999 if mode == "f32" else 0.995)


def _run(model, batch):
    model.zero_grad()
    out = model(**batch)
    out["loss"].backward()
    return float(out["loss"]), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


def test_all_seven_fused_against_generic_and_repeatable(dev):
    import haff  # noqa: F401
    from haff import autograd as A
    from haff import config as hcfg, weights as hw
    from haff.train_model import LisaTrainable
    cfg = hcfg.mid()
    sd = hw.round_to_bf16_(hw.make_state_dict(cfg, 21))
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in _batch(cfg).items()}
    model = LisaTrainable(cfg, sd, dtype=torch.bfloat16, device=dev, lora_dropout=0.0, lora_init_b_zero=False, seed=3,
                          lora_target_modules=ALL7)
    l1, g1 = _run(model, batch)
    l2, g2 = _run(model, batch)
    assert l1 == l2
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k
    try:
        A.FUSED_LORA_QKV = A.FUSED_LORA_OUT = A.FUSED_LORA_GATE_UP = False
        lg, gg = _run(model, batch)
    finally:
        A.FUSED_LORA_QKV = A.FUSED_LORA_OUT = A.FUSED_LORA_GATE_UP = True
    print(f"loss fused {l1:.6f} generic {lg:.6f}")
    assert abs(l1 - lg) <= 1e-2 * max(1.0, abs(lg))
    worst = 0.0
    for k in gg:
        if "lora_" not in k and "embed_tokens" not in k and "lm_head" not in k:
            continue
        rel = ((g1[k].float() - gg[k].float()).norm() / (gg[k].float().norm() + 1e-12)).item()
        worst = max(worst, rel)
        assert rel <= 3e-2, (k, rel)
    print(f"fused vs generic: worst language-model gradient relative L2 {worst:.3e}")


def test_dropout_masks_are_independent_per_adapter(dev):
    import haff  # noqa: F401
    from haff import config as hcfg, weights as hw
    from haff.train_model import LisaTrainable
    cfg = hcfg.mid()
    sd = hw.round_to_bf16_(hw.make_state_dict(cfg, 21))
    model = LisaTrainable(cfg, sd, dtype=torch.bfloat16, device=dev, lora_dropout=0.25, lora_target_modules=ALL7)
    h = torch.randn((300, cfg.llm.hidden), device=dev, dtype=torch.bfloat16)
    for n in (2, 3):
        masks = model._fused_keep(h, n, 0.25)
        assert len(masks) == n
        for i in range(n):
            kept = masks[i].float().mean().item()
            assert abs(kept - 0.75) < 0.02, kept
            assert set(masks[i].unique().tolist()) <= {0.0, 1.0}
            for j in range(i):
                agree = (masks[i] == masks[j]).float().mean().item()
                assert agree < 0.7, agree   # independent: ~0.625 agreement, identical masks give 1
    assert model._fused_keep(h, 3, 0.0) is None
    # a dropout step of the all-seven fused trainer runs and moves every adapter class
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in _batch(cfg).items()}
    model.params["model.layers.0.mlp.down_proj.lora_B"].data.normal_(0, 0.05)
    _, grads = _run(model, batch)
    for n in ("q_proj", "k_proj", "v_proj", "o_proj", "gate_proj", "up_proj", "down_proj"):
        k = f"model.layers.0.{'mlp' if n in ('gate_proj', 'up_proj', 'down_proj') else 'self_attn'}.{n}.lora_B"
        assert torch.isfinite(grads[k]).all() and grads[k].abs().max() > 0, k


def test_all_seven_merged_checkpoint_reproduces_lora_model(dev):
    import haff  # noqa: F401
    from haff import config as hcfg, merge_lora, weights as hw
    from haff.llava import LlamaHip
    from haff.train_model import LisaTrainable
    for cfg in (hcfg.tiny(), hcfg.mid()):
        sd = hw.round_to_bf16_(hw.make_state_dict(cfg, 21))
        m = LisaTrainable(cfg, sd, dtype=torch.bfloat16, device=dev, lora_init_b_zero=False, lora_target_modules=ALL7).eval()
        B, T, H = 2, 24, cfg.llm.hidden
        x = (torch.randn((B * T, H), generator=torch.Generator().manual_seed(5)) * 0.5).to(dev, torch.bfloat16)
        with torch.no_grad():
            ref = m._llm(x.clone(), B, T).float().cpu()
            merged = merge_lora.merge_state_dict(sd, m.state_dict(), 8, 16, torch.bfloat16)
            llm = LlamaHip(merged, cfg.llm, torch.bfloat16, dev)
            got = llm.forward(x.view(B, T, H).clone(), llm.new_cache(B, T)).float().cpu().view(B * T, H)
            qv = LisaTrainable(cfg, sd, dtype=torch.bfloat16, device=dev, lora_init_b_zero=False).eval()
            ref_qv = qv._llm(x.clone(), B, T).float().cpu()
        err = (got - ref).abs().max().item() / ref.abs().max().item()
        print(f"{cfg.llm.hidden}: merged vs LoRA-active hidden rel {err:.3e}")
        assert err <= 3e-2
        assert (ref_qv - ref).abs().max().item() / ref.abs().max().item() > 5 * err   # the five extra adapters act


def test_train_ds_cli_targets_rank_zero_and_resume(dev, tmp_path, capsys):
    import haff  # noqa: F401
    from haff import train_ds
    base = ["--synthetic", "tiny", "--epochs", "1", "--steps_per_epoch", "2", "--grad_accumulation_steps", "1",
            "--batch_size", "2", "--log_base_dir", str(tmp_path), "--mask_hw", "64", "48", "--val_samples", "2", "--lr", "0.0003"]
    argv = base + ["--exp_name", "all7", "--lora_target_modules", ALL7]
    train_ds.main(argv)
    out = capsys.readouterr().out
    assert "in 14 adapters" in out and "saved checkpoint" in out
    blob = torch.load(tmp_path / "all7" / "ckpt_model" / "latest.pt", map_location="cpu", weights_only=False)
    keys = {k for k in blob["params"] if ".lora_" in k}
    assert len(keys) == 28
    for i in range(2):
        for n in ("self_attn.q_proj", "self_attn.k_proj", "self_attn.v_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.up_proj",
                  "mlp.down_proj"):
            assert f"model.layers.{i}.{n}.lora_A" in keys and f"model.layers.{i}.{n}.lora_B" in keys
    i_ep = argv.index("--epochs") + 1
    train_ds.main(argv[:i_ep] + ["2"] + argv[i_ep + 1:])
    out = capsys.readouterr().out
    assert "resume training from" in out and "Epoch: [1][1/2]" in out
    # the same run directory with the default targets: the resume names the extra keys
    default = base + ["--exp_name", "all7", "--epochs", "3"]
    with pytest.raises(ValueError, match=r"extra keys \['model.layers.0.mlp.down_proj.lora_A'"):
        train_ds.main(default)
    capsys.readouterr()
    train_ds.main(base + ["--exp_name", "r0", "--lora_r", "0"])
    out = capsys.readouterr().out
    assert "(LoRA 0 in 0 adapters)" in out and "saved checkpoint" in out
    blob = torch.load(tmp_path / "r0" / "ckpt_model" / "latest.pt", map_location="cpu", weights_only=False)
    assert not any("lora_" in k for k in blob["params"])
