#!/usr/bin/env python3
"""QLoRA against fp16 LoRA fine-tuning on one MI355X: BASELINE.json configs[3] (7B, bench.py's train batch: 8 synthetic 2HANDS samples,
96-id conversations, 1024^2 masks), the fp16 trainer against the fp16 + NF4 trainer (LisaTrainable(load_in_4bit=True)) on the same
weights in one process, their steps alternating round by round, for the default q,v adapters and for all seven targets. A step is
what tools/train_fp16_ab.py times (forward, backward, loss scaling, clip + fused AdamW with the overflow skip, one host read).

Also reported:
  memory   per mode, the bytes its construction left allocated (resident) and torch.cuda.max_memory_allocated over its timed steps
           minus what the OTHER modes keep resident in this process (peak_step);
  kernels  haff_nf4_dequant_f16 and haff_nf4_dequant_t_f16 at the four projection shapes of 7B and 13B: event-timed, warmed, median
           of --kernel-iters launches, as achieved GB/s over the bytes the kernel must move (N K / 2 codes + N K / 16 absmax read,
           2 N K written) and as a fraction of --hbm-tbs.
Prints one JSON line."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import haff  # noqa: E402,F401
from haff import config as hcfg  # noqa: E402
from haff import dist as hdist  # noqa: E402
from haff import quant  # noqa: E402
from haff import train_ops as T  # noqa: E402
from haff import weights as hw  # noqa: E402
from haff.train_model import LisaTrainable  # noqa: E402

ALL7 = "q_proj,k_proj,v_proj,o_proj,gate_proj,up_proj,down_proj"
MODES = (("qv_fp16", "q_proj,v_proj", False), ("qv_nf4", "q_proj,v_proj", True), ("all7_fp16", ALL7, False), ("all7_nf4", ALL7, True))
GEOMS = {"7b": (4096, 11008), "13b": (5120, 13824)}


def _exact_in_all(sd):
    """bf16 values with |v| < 2^-14 zeroed: every weight exact in fp16's normal range (as tools/train_fp16_ab.py)"""
    for k, t in sd.items():
        if torch.is_floating_point(t):
            b = t.to(torch.bfloat16)
            sd[k] = b.masked_fill_(b.abs() < 2.0 ** -14, 0)
    return sd


def kernel_rates(dev, iters, hbm_tbs):
    out = {}
    for geom, (H, F) in GEOMS.items():
        for proj, (N, K) in (("qkv", (3 * H, H)), ("o", (H, H)), ("gate_up", (2 * F, H)), ("down", (H, F))):
            g = torch.Generator(device=dev).manual_seed(N + K)
            q = quant.Nf4Weight(torch.randint(0, 256, (N, K // 2), generator=g, device=dev, dtype=torch.uint8),
                                torch.rand((N, K // 64), generator=g, device=dev) * 0.1 + 0.01)
            w = torch.empty((N, K), dtype=torch.float16, device=dev)
            wt = torch.empty((K, N), dtype=torch.float16, device=dev)
            nbytes = N * K // 2 + N * K // 16 + 2 * N * K
            for name, fn in (("dequant", lambda: q.dequant(out=w)), ("dequant_t", lambda: q.dequant_t(out=wt))):
                for _ in range(5):
                    fn()
                times = []
                for _ in range(iters):
                    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    a.record()
                    fn()
                    b.record()
                    b.synchronize()
                    times.append(a.elapsed_time(b) * 1e-3)
                t = statistics.median(times)
                out[f"{geom}_{proj}_{name}"] = {"N": N, "K": K, "us": round(t * 1e6, 1), "gb_per_s": round(nbytes / t / 1e9, 1),
                                                "of_hbm": round(nbytes / t / (hbm_tbs * 1e12), 3)}
            del q, w, wt
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="7b", choices=["7b", "13b", "tiny", "mid"])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--ids", type=int, default=96)
    ap.add_argument("--mask", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--kernel-iters", type=int, default=30)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM peak in TB/s the kernel fractions are quoted against (MI355X: 8)")
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit("qlora_ab.py measures on an MI355X: no device, no numbers")
    dev = torch.device("cuda:0")
    kernels = kernel_rates(dev, max(args.kernel_iters, 20), args.hbm_tbs)
    torch.cuda.empty_cache()
    cfg = {"7b": hcfg.haff_7b, "13b": hcfg.haff_13b, "tiny": hcfg.tiny, "mid": hcfg.mid}[args.config]()
    sd = _exact_in_all(hw.make_state_dict_device(cfg, 1234, dev, torch.bfloat16))
    batch = bench.make_train_batch(cfg, args.batch, args.ids, (args.mask, args.mask), dev, seed=1234)
    runs = {}
    for name, spec, nf4 in MODES:
        torch.cuda.synchronize()
        before = torch.cuda.memory_allocated()
        model = LisaTrainable(cfg, sd, dtype=torch.float16, device=dev, lora_target_modules=spec, load_in_4bit=nf4)
        named = list(model.named_parameters())
        reducer = T.GradBucketReducer(named)
        runs[name] = {"model": model, "reducer": reducer, "opt": T.BucketAdamW(reducer, named), "scaler": T.DynamicLossScaler(),
                      "losses": [], "peak": 0}
        torch.cuda.synchronize()
        runs[name]["resident"] = torch.cuda.memory_allocated() - before
    del sd
    torch.cuda.empty_cache()

    def step(r):
        model, reducer, opt, scaler = r["model"], r["reducer"], r["opt"], r["scaler"]
        reducer.zero()
        reducer.begin(sync=True)
        out = model(**batch)
        (out["loss"] * scaler.loss_scale).backward()
        reducer.finish()
        gscale = 1.0 / scaler.loss_scale
        norm = T.grad_norm(reducer.grads())
        opt.step(lr=3e-4, gscale=gscale, gscale_dev=T.clip_coef_device(norm * gscale, 1.0), skip_norm=norm)
        if scaler.update_scale(not bool(torch.isfinite(norm).item())):
            opt.unstep()
        r["losses"].append(out["loss"].detach())

    for r in runs.values():
        for _ in range(args.warmup):
            step(r)
    sps = {k: [] for k in runs}
    for _ in range(args.rounds):
        for name, r in runs.items():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            elapsed = hdist.timed_steps(lambda: step(r), args.steps, dev)
            sps[name].append(args.batch * args.steps / elapsed)
            others = sum(o["resident"] for n, o in runs.items() if n != name)
            r["peak"] = max(r["peak"], torch.cuda.max_memory_allocated() - others)
    med = {k: statistics.median(v) for k, v in sps.items()}
    gb = 2.0 ** 30
    res = {"config": args.config, "batch": args.batch, "steps": args.steps, "rounds": args.rounds, "warmup": args.warmup,
           "samples_per_s": {k: [round(x, 2) for x in v] for k, v in sps.items()},
           "samples_per_s_median": {k: round(v, 2) for k, v in med.items()},
           "nf4_over_fp16": {"qv": round(med["qv_nf4"] / med["qv_fp16"], 4), "all7": round(med["all7_nf4"] / med["all7_fp16"], 4)},
           "resident_gb": {k: round(r["resident"] / gb, 2) for k, r in runs.items()},
           "peak_step_gb": {k: round(r["peak"] / gb, 2) for k, r in runs.items()},
           "frozen_llama_gb": {k: round((sum(L[n].nbytes if r["model"].load_in_4bit else 2 * L[n].numel() * 2
                                             for L in r["model"].base.llm.layers for n in ("wqkv", "wo", "wgu", "wd"))
                                         + sum(t.numel() * 2 for t in r["model"].nf4_scratch.values())) / gb, 2) for k, r in runs.items()},
           "skipped_steps": {k: r["scaler"].skipped_steps for k, r in runs.items()},
           "loss_first_last": {k: [round(float(r["losses"][0]), 4), round(float(r["losses"][-1]), 4)] for k, r in runs.items()},
           "hbm_tbs_assumed": args.hbm_tbs, "dequant_kernels": kernels}
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
