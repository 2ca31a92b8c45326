#!/usr/bin/env python3
"""What the data loader costs a fine-tune step on one MI355X, and what --device_ingest gets back: BASELINE.json configs[3] (7B, bf16,
bench.py's train batch of 8 samples per step) fed three ways in ONE process, alternating round by round:

  tensor  one batch already resident as tensors, re-used every step (what bench.py --mode train and the published rates measure)
  host    train_ds.py's default loader: collate_fn([dataset[i] ...]) on the main thread inside the step loop, then the copies
  device  train_ds.py --device_ingest: train_ingest.Prefetcher + DeviceIngest.batch

The records are generated here: random uint8 frames (1024 x 1024, and 256 x 456) with one wavy closed contour of about 800 vertices
per hand, masks at the frame's size; prompts from the dataset's own templates through the byte tokenizer. A step is what
bench.py --mode train times (forward, backward, clip + fused AdamW); the rates are samples/s INCLUDING the data time. All three feeds
carry the same shapes (the tensor feed re-uses the first host-built batch). Writes one JSON file (--out).

--fill-only: no model; launches haff_fill_contours_u8 on 2 planes x 8 samples at 1024 x 1024 back to back (for a kernel trace run of
its own) and reports the wall time per call between two device synchronisations beside the bytes it writes."""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import haff  # noqa: E402,F401
from haff import aff_dataset, checkpoint  # noqa: E402
from haff import config as hcfg  # noqa: E402
from haff import dist as hdist  # noqa: E402
from haff import ops, train_ds  # noqa: E402
from haff import train_ops as T  # noqa: E402
from haff import weights as hw  # noqa: E402
from haff.train_ingest import DeviceIngest, Prefetcher  # noqa: E402
from haff.train_model import LisaTrainable  # noqa: E402


def wavy_contour(cx, cy, r, n=800, lobes=9, phase=0.0):
    t = 2 * math.pi * np.arange(n) / n
    rad = r * (1 + 0.2 * np.sin(lobes * t + phase))
    return np.stack([cx + rad * np.cos(t), cy + rad * np.sin(t)], 1).astype(np.int32).tolist()


def make_records(n, hw_, seed):
    rng = np.random.default_rng(seed)
    H, W = hw_
    acts = ["cut the bread", "open the drawer", "pour water into the cup", "hold the pan", "stir the pot", "lift the lid"]
    recs = []
    for i in range(n):
        recs.append({"narration": acts[i % len(acts)], "inpainted": rng.integers(0, 256, (H, W, 3), dtype=np.uint8),
                     "taxonomy": [0.0, 0.0, 1.0, 0.0],
                     "masks": {"aff_left": [wavy_contour(W * 0.32, H * 0.45, min(H, W) * 0.22, lobes=9, phase=0.3 * i)],
                               "aff_right": [wavy_contour(W * 0.68, H * 0.55, min(H, W) * 0.25, lobes=7, phase=0.2 * i)],
                               "original_size": (H, W)}})
    return recs


def fill_only(args, dev):
    hw_ = (1024, 1024)
    recs = make_records(8, hw_, 0)
    planes = [r["masks"][k] for r in recs for k in ("aff_left", "aff_right")]
    out = torch.empty((len(planes),) + hw_, dtype=torch.uint8, device=dev)
    for _ in range(5):
        ops.fill_contours(planes, hw_, dev, out=out)
    ones = int(out.sum(dtype=torch.int64))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.fill_calls):
        ops.fill_contours(planes, hw_, dev, out=out)
    torch.cuda.synchronize()
    wall_us = 1e6 * (time.perf_counter() - t0) / args.fill_calls
    n_vert = sum(len(c) for p in planes for c in p)
    return {"planes": len(planes), "hw": list(hw_), "vertices": n_vert, "calls": args.fill_calls,
            "bytes_zeroed": out.numel(), "bytes_set_to_one": ones,
            "wall_us_per_call_including_host_packing_and_upload": round(wall_us, 1)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="7b", choices=["7b", "13b", "tiny", "mid"])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="1024x1024,256x456")
    ap.add_argument("--out", default=os.path.join("profiles", "train_ingest_ab_7b_b8.json"))
    ap.add_argument("--fill-only", action="store_true")
    ap.add_argument("--fill-calls", type=int, default=200)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    if args.fill_only:
        res = {"fill_kernel": fill_only(args, dev)}
        print(json.dumps(res))
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        return
    cfg = {"7b": hcfg.haff_7b, "13b": hcfg.haff_13b, "tiny": hcfg.tiny, "mid": hcfg.mid}[args.config]()
    tok = checkpoint.ByteTokenizer(cfg)
    sd = hw.make_state_dict_device(cfg, 1234, dev, torch.bfloat16)
    model = LisaTrainable(cfg, sd, dtype=torch.bfloat16, device=dev)
    del sd
    torch.cuda.empty_cache()
    named = list(model.named_parameters())
    reducer = T.GradBucketReducer(named)
    opt = T.BucketAdamW(reducer, named)
    losses = []

    def train_step(batch):
        reducer.zero()
        reducer.begin(sync=True)
        out = model(**batch)
        out["loss"].backward()
        reducer.finish()
        opt.step(lr=3e-4, gscale=1.0, gscale_dev=T.clip_coef_device(T.grad_norm(reducer.grads()), 1.0))
        losses.append(out["loss"].detach())

    ingest = DeviceIngest(cfg, dev, torch.bfloat16)
    result = {"config": args.config, "dtype": "bf16", "batch": args.batch, "rounds": args.rounds, "steps": args.steps,
              "warmup": args.warmup, "tokenizer": "byte", "host_cpus": os.cpu_count(), "torch_threads": torch.get_num_threads(),
              "sizes": {}}
    for size in args.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        recs = make_records(16, (H, W), seed=H)
        host_ds = aff_dataset.AffRecordsDataset(recs, cfg, seed=1)
        dev_ds = aff_dataset.AffRecordsDataset(recs, cfg, seed=1)
        pos = {"host": 0}

        def host_batch():
            b = train_ds.collate_fn([host_ds[pos["host"] + j] for j in range(args.batch)], tok, 3000)
            pos["host"] += args.batch
            return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
        fixed = host_batch()
        pf = Prefetcher(dev_ds.raw_item, 0, args.batch, prepare=lambda raws: ingest.text(raws, tok, 3000, "llava_v1"))

        def device_batch():
            raws, text = pf.get()
            return ingest.batch(raws, tok, 3000, "llava_v1", text=text)
        feeds = {"tensor": lambda: fixed, "host": host_batch, "device": device_batch}
        try:
            for feed in feeds.values():
                for _ in range(args.warmup):
                    train_step(feed())
            sps = {k: [] for k in feeds}
            data_ms = {k: [] for k in feeds}
            for _ in range(args.rounds):
                for name, feed in feeds.items():
                    spent = [0.0]

                    def step():
                        t0 = time.perf_counter()
                        batch = feed()
                        spent[0] += time.perf_counter() - t0
                        train_step(batch)
                    elapsed = hdist.timed_steps(step, args.steps, dev)
                    sps[name].append(args.batch * args.steps / elapsed)
                    data_ms[name].append(1e3 * spent[0] / args.steps)
        finally:
            pf.close()
        med = {k: statistics.median(v) for k, v in sps.items()}
        result["sizes"][size] = {
            "ids_per_conversation": int(fixed["input_ids"].shape[1]), "mask_hw": [H, W], "vertices_per_contour": len(recs[0]["masks"]["aff_left"][0]),
            "samples_per_s": {k: [round(x, 2) for x in v] for k, v in sps.items()},
            "samples_per_s_median": {k: round(v, 2) for k, v in med.items()},
            "main_thread_ms_per_step_getting_the_batch": {k: [round(x, 1) for x in v] for k, v in data_ms.items()},
            "device_over_host": round(med["device"] / med["host"], 3), "device_over_tensor": round(med["device"] / med["tensor"], 3),
            "host_over_tensor": round(med["host"] / med["tensor"], 3), "host_fills": ingest.host_fills}
    result["loss_first_last"] = [round(float(losses[0]), 4), round(float(losses[-1]), 4)]
    result["peak_hbm_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
