#!/usr/bin/env python3
"""fp16 against bf16 LoRA fine-tuning on one MI355X: BASELINE.json configs[3] (7B, bench.py's train batch: 8 synthetic 2HANDS samples,
96-id conversations, 1024^2 masks), the two trainers on the same weights in one process, their steps alternating round by round.
A step is what bench.py --mode train times (forward, backward, clip + fused AdamW over the gradient buckets); the fp16 step adds
train_ds.py's loss scaling: the scaled loss, the overflow-skipping update and the one host read of the gradient norm per step.
Prints one JSON line: samples/s per mode (per round and median), fp16 / bf16, and the fp16 run's skipped steps and final scale."""
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
from haff import train_ops as T  # noqa: E402
from haff import weights as hw  # noqa: E402
from haff.train_model import LisaTrainable  # noqa: E402


def _exact_in_all(sd):
    """bf16 values with |v| < 2^-14 zeroed: one weight set both modes represent exactly (as tools/fp16_ab.py)"""
    for k, t in sd.items():
        if torch.is_floating_point(t):
            b = t.to(torch.bfloat16)
            sd[k] = b.masked_fill_(b.abs() < 2.0 ** -14, 0)
    return sd


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="7b", choices=["7b", "13b", "tiny", "mid"])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--ids", type=int, default=96)
    ap.add_argument("--mask", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    cfg = {"7b": hcfg.haff_7b, "13b": hcfg.haff_13b, "tiny": hcfg.tiny, "mid": hcfg.mid}[args.config]()
    sd = _exact_in_all(hw.make_state_dict_device(cfg, 1234, dev, torch.bfloat16))
    batch = bench.make_train_batch(cfg, args.batch, args.ids, (args.mask, args.mask), dev, seed=1234)
    runs = {}
    for name, dtype in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        model = LisaTrainable(cfg, sd, dtype=dtype, device=dev)
        named = list(model.named_parameters())
        reducer = T.GradBucketReducer(named)
        runs[name] = {"model": model, "reducer": reducer, "opt": T.BucketAdamW(reducer, named),
                      "scaler": T.DynamicLossScaler() if dtype == torch.float16 else None, "losses": []}
    del sd
    torch.cuda.empty_cache()

    def step(r):
        model, reducer, opt, scaler = r["model"], r["reducer"], r["opt"], r["scaler"]
        reducer.zero()
        reducer.begin(sync=True)
        out = model(**batch)
        (out["loss"] * scaler.loss_scale if scaler else out["loss"]).backward()
        reducer.finish()
        gscale = 1.0 / scaler.loss_scale if scaler else 1.0
        norm = T.grad_norm(reducer.grads())
        opt.step(lr=3e-4, gscale=gscale, gscale_dev=T.clip_coef_device(norm * gscale, 1.0), skip_norm=norm if scaler else None)
        if scaler is not None and scaler.update_scale(not bool(torch.isfinite(norm).item())):
            opt.unstep()
        r["losses"].append(out["loss"].detach())

    for r in runs.values():
        for _ in range(args.warmup):
            step(r)
    sps = {k: [] for k in runs}
    for _ in range(args.rounds):
        for name, r in runs.items():
            elapsed = hdist.timed_steps(lambda: step(r), args.steps, dev)
            sps[name].append(args.batch * args.steps / elapsed)
    med = {k: statistics.median(v) for k, v in sps.items()}
    sc = runs["fp16"]["scaler"]
    res = {"config": args.config, "batch": args.batch, "steps": args.steps, "rounds": args.rounds, "warmup": args.warmup,
           "samples_per_s": {k: [round(x, 2) for x in v] for k, v in sps.items()},
           "samples_per_s_median": {k: round(v, 2) for k, v in med.items()},
           "fp16_over_bf16": round(med["fp16"] / med["bf16"], 4),
           "fp16_skipped_steps": sc.skipped_steps, "fp16_loss_scale": sc.loss_scale,
           "loss_first_last": {k: [round(float(r["losses"][0]), 4), round(float(r["losses"][-1]), 4)] for k, r in runs.items()},
           "peak_hbm_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
