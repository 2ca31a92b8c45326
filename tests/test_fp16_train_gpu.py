"""fp16 fine-tuning end to end: LisaTrainable(dtype=torch.float16) against the CPU oracle's model_forward under autograd (and closer
to it than the bf16 mode on the same weights), its inference outputs against the fp16 inference mode, the loss-scaled loop
(overflow skips, hysteresis, halving, bitwise-unchanged state), repeatability, and train_ds --precision fp16 (scale logged and
checkpointed, resume, 2 + 2 steps == 4 steps, merge into the fp16 inference model)."""
import os
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
BF16_CLASS_TOL = {"lora_A": 3e-2, "lora_B": 3e-2, "embed_tokens": 2e-2, "lm_head": 1.2e-2, "text_hidden_fcs": 0.2,
                  "decoder.output_upscaling": 3e-2}   # the bf16 test's per-class bounds (tests/test_train_gpu.py)


def _exact_in_all(sd):
    """bf16 values with |v| < 2^-14 zeroed: every weight exact in bf16, fp16 (normal range) and fp32."""
    for k, t in sd.items():
        if torch.is_floating_point(t):
            b = t.to(torch.bfloat16)
            sd[k] = b.masked_fill_(b.abs() < 2.0 ** -14, 0).float()
    return sd


def _batch(cfg, seed=0):
    sys.path.insert(0, HERE)
    from test_train_gpu import make_batch
    b = make_batch(cfg, seed=seed)
    b["images"] = _exact_in_all({"x": b["images"]})["x"]
    b["images_clip"] = _exact_in_all({"x": b["images_clip"]})["x"]
    return b


def _class(key):
    sys.path.insert(0, HERE)
    from test_train_gpu import grad_class
    return grad_class(key)


def _errors(dev, cfg, sd, batch, dtype):
    """losses and per-tensor relative L2 gradient errors of LisaTrainable(dtype) against the oracle under autograd"""
    from haff.train_model import LisaTrainable
    from oracle import lisa_oracle as O
    model = LisaTrainable(cfg, sd, dtype=dtype, device=dev, lora_dropout=0.0, lora_init_b_zero=False, seed=3)
    osd = {k: v.clone() for k, v in sd.items()}
    lora = {}
    for k, p in model.named_parameters():
        t = p.detach().float().cpu().clone().requires_grad_(True)
        (lora if "lora_" in k else osd)[k] = t
    ref = O.lisa_model_forward(osd, cfg, batch, lora=lora)
    ref["loss"].backward()
    out = model(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()})
    out["loss"].backward()
    losses = {k: (float(out[k]), float(ref[k])) for k in ref}
    rel = {}
    for k, p in model.named_parameters():
        r = (lora[k] if "lora_" in k else osd[k]).grad
        if r is None or p.grad is None or r.abs().max().item() < 1e-6:
            continue
        rel[k] = ((p.grad.float().cpu() - r).norm() / (r.norm() + 1e-12)).item()
    return losses, rel


@pytest.mark.parametrize("geom", ["tiny", "mid"])
def test_fp16_forward_backward_matches_oracle_and_beats_bf16(dev, geom):
    import haff  # noqa: F401
    from haff import config as hcfg, weights as hw
    cfg = getattr(hcfg, geom)()
    sd = _exact_in_all(hw.make_state_dict(cfg, 21))
    batch = _batch(cfg)
    l16, r16 = _errors(dev, cfg, sd, batch, torch.float16)
    lbf, rbf = _errors(dev, cfg, sd, batch, torch.bfloat16)
    for k, (a, b) in l16.items():
        print(f"fp16 {k}: hip {a:.6f} oracle {b:.6f} (bf16 {lbf[k][0]:.6f})")
        assert abs(a - b) <= 3e-2 * max(1.0, abs(b)), k
    assert len(r16) > 100
    by16, bybf = {}, {}
    for k, v in r16.items():
        assert v <= 0.25, (k, v)
        by16[_class(k)] = max(by16.get(_class(k), 0.0), v)
        bybf[_class(k)] = max(bybf.get(_class(k), 0.0), rbf[k])
    print("per class worst relative L2, fp16 / bf16: " + ", ".join(f"{c} {by16[c]:.3e} / {bybf[c]:.3e}" for c in sorted(by16)))
    for c, v in by16.items():
        assert v <= BF16_CLASS_TOL.get(c, 0.25), (c, v)
        assert v < bybf[c], f"fp16 class {c} ({v:.3e}) not closer to the oracle than bf16 ({bybf[c]:.3e})"


def test_fp16_trainer_inference_matches_fp16_inference_mode(dev):
    """inference=True of an fp16 trainer (LoRA B = 0: the adapted model IS the base) runs the fp16 inference mode's frozen stacks:
    its Llama hidden states equal LlamaHip's fp16 forward on the same weights, and the teacher-forced masks / taxonomy come out."""
    import haff  # noqa: F401
    from haff import config as hcfg, weights as hw
    from haff.train_model import LisaTrainable
    cfg = hcfg.tiny()
    sd = _exact_in_all(hw.make_state_dict(cfg, 5))
    model = LisaTrainable(cfg, sd, dtype=torch.float16, device=dev, lora_dropout=0.0).eval()
    B, T, H = 2, 24, cfg.llm.hidden
    x = (torch.randn((B * T, H), generator=torch.Generator().manual_seed(5)) * 0.5).to(dev, torch.float16)
    with torch.no_grad():
        got = model._llm(x.clone(), B, T).float().cpu()
        llm = model.base.llm
        ref = llm.forward(x.view(B, T, H).clone(), llm.new_cache(B, T)).float().cpu().view(B * T, H)
    err = (got - ref).abs().max().item() / ref.abs().max().item()
    print(f"fp16 trainer vs fp16 inference Llama hidden: rel {err:.3e}")
    assert err <= 1e-2
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in _batch(cfg, 2).items()}
    with torch.no_grad():
        out = model(**{**batch, "inference": True})
    assert out["pred_masks_left"].shape == (2, 1, 100, 90) and out["pred_taxonomies"].shape == (2, 1, 4)
    assert torch.isfinite(out["pred_masks_left"]).all() and torch.isfinite(out["pred_masks_right"]).all()


def _loop(dev, init_scale=2.0 ** 16, steps=6, seed=22, base_lr=3e-4):
    from haff import config as hcfg, weights as hw
    from haff import train_ops as T
    from haff.train_model import LisaTrainable
    cfg = hcfg.tiny()
    sd = _exact_in_all(hw.make_state_dict(cfg, seed))
    model = LisaTrainable(cfg, sd, dtype=torch.float16, device=dev, lora_dropout=0.0, lora_init_b_zero=False)
    sys.path.insert(0, HERE)
    from test_train_gpu import make_batch
    batch = {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in make_batch(cfg, seed=1).items()}
    named = model.named_parameters()
    reducer = T.GradBucketReducer(named)
    opt = T.BucketAdamW(reducer, named)
    scaler = T.DynamicLossScaler(init_scale=init_scale)
    rec = []
    taken = 0
    for _ in range(steps):
        reducer.zero()
        reducer.begin(sync=True)
        out = model(**batch)
        (out["loss"] * scaler.loss_scale).backward()
        reducer.finish()
        gscale = 1.0 / scaler.loss_scale
        norm = T.grad_norm(reducer.grads())
        before = [(b["master"].clone(), b["m"].clone(), b["v"].clone()) for b in opt.buckets]
        lr = T.warmup_decay_lr(taken, 100, base_lr, warmup_steps=0)
        opt.step(lr=lr, gscale=gscale, gscale_dev=T.clip_coef_device(norm * gscale, 1.0), skip_norm=norm)
        scale_used = scaler.loss_scale
        skipped = scaler.update_scale(not bool(torch.isfinite(norm).item()))
        if skipped:
            opt.unstep()
            for b, (ma, m, v) in zip(opt.buckets, before):
                assert torch.equal(b["master"], ma) and torch.equal(b["m"], m) and torch.equal(b["v"], v)
        else:
            taken += 1
        rec.append((float(out["loss"]), scale_used, skipped, opt.step_count))
    return rec, model, opt


def test_fp16_loop_with_loss_scaling_lowers_the_loss(dev):
    import haff  # noqa: F401
    rec, _, _ = _loop(dev)
    print(rec)
    taken = [r for r in rec if not r[2]]
    assert len(taken) >= 4 and rec[-1][0] < rec[0][0]


def test_forced_overflow_skips_steps_with_hysteresis_then_halving(dev):
    import haff  # noqa: F401
    rec, model, opt = _loop(dev, init_scale=2.0 ** 40, steps=4)
    print(rec)
    # 2^40 times the loss overflows every f16 gradient path: step 1 spends the hysteresis (scale kept), step 2 halves
    assert rec[0][2] and rec[0][1] == 2.0 ** 40
    assert rec[1][2] and rec[1][1] == 2.0 ** 40
    assert rec[2][1] == 2.0 ** 39
    assert all(r[3] == sum(1 for q in rec[:i + 1] if not q[2]) for i, r in enumerate(rec))   # skipped steps do not count
    for b in opt.buckets:
        if b["lp"] is not None:
            assert torch.equal(b["lp"], b["master"].to(b["lp"].dtype))


def test_fp16_steps_are_bitwise_repeatable(dev):
    import haff  # noqa: F401
    r1, m1, _ = _loop(dev, steps=2)
    r2, m2, _ = _loop(dev, steps=2)
    assert r1 == r2
    for (k, a), (_, b) in zip(m1.named_parameters(), m2.named_parameters()):
        assert torch.equal(a, b), k


def test_train_ds_fp16_cli_scale_checkpoint_resume_and_merge(dev, tmp_path, capsys):
    import haff  # noqa: F401
    from haff import train_ds
    common = ["--synthetic", "tiny", "--grad_accumulation_steps", "1", "--batch_size", "2", "--mask_hw", "64", "48",
              "--lora_dropout", "0", "--no_eval", "--lr", "0.0003", "--precision", "fp16", "--print_freq", "1"]
    train_ds.main(common + ["--epochs", "1", "--steps_per_epoch", "4", "--log_base_dir", str(tmp_path / "a"), "--exp_name", "x"])
    out = capsys.readouterr().out
    assert "LossScale 65536" in out and "Epoch: [0][4/4]" in out
    train_ds.main(common + ["--epochs", "1", "--steps_per_epoch", "2", "--log_base_dir", str(tmp_path / "b"), "--exp_name", "x"])
    blob = torch.load(tmp_path / "b" / "x" / "ckpt_model" / "latest.pt", weights_only=False)
    assert blob["loss_scaler"]["cur_scale"] == 65536.0 and blob["loss_scaler"]["cur_iter"] == 2
    assert all(v.dtype in (torch.float16, torch.float32) for v in blob["params"].values())
    assert any(v.dtype == torch.float16 for v in blob["params"].values())
    train_ds.main(common + ["--epochs", "2", "--steps_per_epoch", "2", "--log_base_dir", str(tmp_path / "b"), "--exp_name", "x"])
    out = capsys.readouterr().out
    assert "resume training from" in out and "LossScale" in out
    a = torch.load(tmp_path / "a" / "x" / "ckpt_model" / "latest.pt", weights_only=False)
    b = torch.load(tmp_path / "b" / "x" / "ckpt_model" / "latest.pt", weights_only=False)
    assert b["loss_scaler"]["cur_iter"] == 4 and a["loss_scaler"] == b["loss_scaler"]
    for k in a["params"]:
        assert torch.equal(a["params"][k], b["params"][k]), k
    for k in a["optim"]:
        for f in ("master", "m", "v"):
            assert torch.equal(a["optim"][k][f], b["optim"][k][f]), (k, f)
    # the fp16 checkpoint merges and serves in the fp16 inference mode
    from haff import checkpoint, config as hcfg, merge_lora
    from haff.lisa import LisaMI355
    cfg = hcfg.tiny()
    sd = checkpoint.synthetic_state_dict(cfg, 1234, dev, torch.float16)
    merged = merge_lora.merge_state_dict(sd, b["params"], 8, 16, torch.float16)
    merged.update({k: v for k, v in sd.items() if k not in merged})   # the CLIP tower is not part of the merged export
    m = LisaMI355(cfg, merged, dtype=torch.float16, device=dev)
    assert m.dtype == torch.float16
