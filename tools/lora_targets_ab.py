#!/usr/bin/env python3
"""LoRA targets on one MI355X: BASELINE.json configs[3] (7B, bench.py's train batch: 8 synthetic 2HANDS samples, 96-id
conversations, 1024^2 masks) with three trainers on the same weights in one process, their steps alternating round by round:
  qv          --lora_target_modules q_proj,v_proj (the default: the fused q|k|v node with two adapters)
  all7_fused  all seven projections on the fused nodes (q|k|v with three adapters, o / down with haff_lora_out, gate|up with
              haff_lora_gu_swiglu)
  all7_generic all seven on the generic composition (FUSED_LORA_QKV / FUSED_LORA_OUT / FUSED_LORA_GATE_UP off: LinearFn,
              scale, add nodes per adapter)
A step is what bench.py --mode train times (forward, backward, clip + fused AdamW over the gradient buckets), with the default
lora_dropout 0.05. Prints one JSON line: samples/s per mode (per round and median) and the ratios."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402
import haff  # noqa: E402,F401
from haff import autograd as A  # noqa: E402
from haff import config as hcfg  # noqa: E402
from haff import dist as hdist  # noqa: E402
from haff import train_ops as T  # noqa: E402
from haff import weights as hw  # noqa: E402
from haff.train_model import LisaTrainable  # noqa: E402

ALL7 = "q_proj,k_proj,v_proj,o_proj,gate_proj,up_proj,down_proj"
MODES = (("qv", "q_proj,v_proj", True), ("all7_fused", ALL7, True), ("all7_generic", ALL7, False))


def _fused(on):
    A.FUSED_LORA_QKV = A.FUSED_LORA_OUT = A.FUSED_LORA_GATE_UP = on


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
    sd = hw.make_state_dict_device(cfg, 1234, dev, torch.bfloat16)
    batch = bench.make_train_batch(cfg, args.batch, args.ids, (args.mask, args.mask), dev, seed=1234)
    runs = {}
    for name, spec, fused in MODES:
        model = LisaTrainable(cfg, sd, dtype=torch.bfloat16, device=dev, lora_target_modules=spec)
        named = list(model.named_parameters())
        reducer = T.GradBucketReducer(named)
        runs[name] = {"model": model, "reducer": reducer, "opt": T.BucketAdamW(reducer, named), "fused": fused, "losses": [],
                      "lora_params": sum(p.numel() for k, p in named if "lora_" in k)}
    del sd
    torch.cuda.empty_cache()

    def step(r):
        _fused(r["fused"])
        model, reducer, opt = r["model"], r["reducer"], r["opt"]
        reducer.zero()
        reducer.begin(sync=True)
        out = model(**batch)
        out["loss"].backward()
        reducer.finish()
        norm = T.grad_norm(reducer.grads())
        opt.step(lr=3e-4, gscale=1.0, gscale_dev=T.clip_coef_device(norm, 1.0))
        r["losses"].append(out["loss"].detach())

    try:
        for r in runs.values():
            for _ in range(args.warmup):
                step(r)
        sps = {k: [] for k in runs}
        for _ in range(args.rounds):
            for name, r in runs.items():
                elapsed = hdist.timed_steps(lambda: step(r), args.steps, dev)
                sps[name].append(args.batch * args.steps / elapsed)
    finally:
        _fused(True)
    med = {k: statistics.median(v) for k, v in sps.items()}
    res = {"config": args.config, "batch": args.batch, "steps": args.steps, "rounds": args.rounds, "warmup": args.warmup,
           "lora_params": {k: r["lora_params"] for k, r in runs.items()},
           "samples_per_s": {k: [round(x, 2) for x in v] for k, v in sps.items()},
           "samples_per_s_median": {k: round(v, 2) for k, v in med.items()},
           "all7_fused_over_qv": round(med["all7_fused"] / med["qv"], 4),
           "all7_fused_over_generic": round(med["all7_fused"] / med["all7_generic"], 4),
           "loss_first_last": {k: [round(float(r["losses"][0]), 4), round(float(r["losses"][-1]), 4)] for k, r in runs.items()},
           "peak_hbm_gb": round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
