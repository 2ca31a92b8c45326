#!/usr/bin/env python3
"""What the training augmentation costs a fine-tune step on one MI355X: the setup of tools/train_ingest_ab.py (BASELINE.json
configs[3]: 7B, bf16, 8 samples per step, generated records at 1024 x 1024 and 256 x 456) fed three ways in ONE process, alternating
round by round:

  device      train_ds.py --device_ingest
  device_aug  train_ds.py --device_ingest --aug_flip 0.5 --aug_jitter 0.25   (csrc/frame_augment.hip)
  host_aug    train_ds.py --aug_flip 0.5 --aug_jitter 0.25                   (the host loader: Pillow on the main thread)

--crop P adds the third augmentation to the alternation, on records that carry object contours too:

  device_crop train_ds.py --device_ingest --aug_flip 0.5 --aug_crop P --aug_jitter 0.25   (csrc/frame_crop.hip as well)
  host_crop   train_ds.py --aug_flip 0.5 --aug_crop P --aug_jitter 0.25

The rates are samples/s INCLUDING the data time; a step is what bench.py --mode train times. Writes one JSON file (--out).

--kernels-only: no model; runs the stats and augment passes on 8 frames of 1024 x 1024 (all mirrored and jittered) and the plane
mirror on 16 planes back to back, for a kernel trace run of its own, and reports the wall time per call between two device
synchronisations beside the bytes each moves."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from train_ingest_ab import make_records, wavy_contour  # noqa: E402  (also puts the repository root on sys.path and imports haff)
from haff import aff_dataset, checkpoint  # noqa: E402
from haff import config as hcfg  # noqa: E402
from haff import dist as hdist  # noqa: E402
from haff import ops, train_ds  # noqa: E402
from haff import train_ops as T  # noqa: E402
from haff import weights as hw  # noqa: E402
from haff.train_ingest import DeviceIngest, Prefetcher  # noqa: E402
from haff.train_model import LisaTrainable  # noqa: E402

P_FLIP, P_JITTER = 0.5, 0.25


def kernels_only(args, dev):
    B, H, W = 8, 1024, 1024
    frames = torch.randint(0, 256, (B, H, W, 3), dtype=torch.uint8, device=dev)
    planes = torch.randint(0, 2, (2 * B, H, W), dtype=torch.uint8, device=dev)
    flags, factors = ops.augment_table([{"flip": True, "jitter": (0.7, 1.3, 0.9)}] * B, dev)
    pflags = torch.ones((2 * B,), dtype=torch.int32, device=dev)
    sums, out, pout = torch.empty((B,), dtype=torch.int64, device=dev), torch.empty_like(frames), torch.empty_like(planes)

    def timed(fn):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.calls):
            fn()
        torch.cuda.synchronize()
        return round(1e6 * (time.perf_counter() - t0) / args.calls, 1)
    n = frames.numel()
    # the object crop: every sample mirrored and cropped, boxes of 539 ... 677 px squares as the generated records of main() give
    boxes = [{"x0": 217 + 2 * i, "y0": 234 + 9 * i, "cw": 539 + 19 * i, "ch": 522 - 19 * i, "px": 0, "py": (17 + 38 * i) // 2,
              "S": 539 + 19 * i} for i in range(B)]
    flips = [True] * B
    desc = ops.crop_descriptor(boxes, flips, (H, W))
    pboxes, pflips = [b for b in boxes for _ in range(2)], flips * 2
    pdesc = ops.crop_descriptor(pboxes, pflips, (H, W))
    planes4 = planes[..., None]
    pout4 = torch.empty_like(planes4)
    crop = {"boxes_S": [b["S"] for b in boxes], "descriptor_bytes": 4 * desc.numel(),
            "crop_frames": {"bytes_written": n, "wall_us_per_call":
                            timed(lambda: ops.crop_resample(frames, boxes, flips, out=out, desc=desc))},
            "crop_planes": {"bytes_written": planes.numel(), "wall_us_per_call":
                            timed(lambda: ops.crop_resample(planes4, pboxes, pflips, out=pout4, desc=pdesc))},
            "crop_frames_with_descriptor_built_per_call": {"wall_us_per_call":
                                                           timed(lambda: ops.crop_resample(frames, boxes, flips, out=out))}}
    t0 = time.perf_counter()
    for S in range(300, 364):
        ops.crop_table(S, 1024 + (S & 1))             # 64 tables nobody has cached
    crop["table_build_ms_per_1024_row_table"] = round(1e3 * (time.perf_counter() - t0) / 64, 2)
    return {"frames": [B, H, W, 3], "planes": [2 * B, H, W], "calls": args.calls, "crop": crop,
            "jitter_stats": {"bytes_read": n, "wall_us_per_call": timed(lambda: ops.jitter_stats(frames, flags, factors, out=sums))},
            "augment": {"bytes_read": n, "bytes_written": n,
                        "wall_us_per_call": timed(lambda: ops.augment_u8(frames, flags, factors, sums, out=out))},
            "flip_planes": {"bytes_read": planes.numel(), "bytes_written": planes.numel(),
                            "wall_us_per_call": timed(lambda: ops.flip_planes(planes, pflags, out=pout))}}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="7b", choices=["7b", "13b", "tiny", "mid"])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--sizes", default="1024x1024,256x456")
    ap.add_argument("--feeds", default=None, help="a subset runs alone, e.g. under a kernel trace (default: every feed)")
    ap.add_argument("--crop", type=float, default=0.0, help="also feed with --aug_crop P (device_crop, host_crop); 0.6667 is 2HANDS' share")
    ap.add_argument("--out", default=os.path.join("profiles", "train_aug_ab_7b_b8.json"))
    ap.add_argument("--kernels-only", action="store_true")
    ap.add_argument("--calls", type=int, default=200)
    args = ap.parse_args(argv)
    if args.feeds is None:
        args.feeds = "device,device_aug,host_aug" + (",device_crop,host_crop" if args.crop > 0.0 else "")
    dev = torch.device("cuda:0")
    if args.kernels_only:
        res = {"augment_kernels": kernels_only(args, dev)}
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
              "warmup": args.warmup, "tokenizer": "byte", "aug_flip": P_FLIP, "aug_jitter": P_JITTER, "aug_crop": args.crop, "host_cpus": os.cpu_count(),
              "torch_threads": torch.get_num_threads(), "sizes": {}}
    for size in args.sizes.split(","):
        H, W = (int(v) for v in size.split("x"))
        recs = make_records(16, (H, W), seed=H)
        for i, r in enumerate(recs):      # the objects: inside the frame, as findContours gives them; another box per record
            m = r["masks"]
            m["obj_left"] = [wavy_contour(W * 0.4, H * (0.4 + 0.01 * i), min(H, W) * 0.12, lobes=5, phase=0.1 * i)]
            m["obj_right"] = [wavy_contour(W * (0.55 + 0.01 * i), H * 0.55, min(H, W) * 0.12, lobes=6, phase=0.2 * i)]
        aug = {"aug_flip": P_FLIP, "aug_jitter": P_JITTER}
        crop = dict(aug, aug_crop=args.crop)
        kwargs = {"device": {}, "device_aug": aug, "host_aug": aug, "device_crop": crop, "host_crop": crop}
        names = args.feeds.split(",")
        datasets = {k: aff_dataset.AffRecordsDataset(recs, cfg, seed=1, **kwargs[k]) for k in names}
        pos = {k: 0 for k in names}
        seen = {"flip": 0, "jitter": 0, "samples": 0, "crop": 0, "crop_samples": 0}

        def host_batch(name):
            b = train_ds.collate_fn([datasets[name][pos[name] + j] for j in range(args.batch)], tok, 3000)
            pos[name] += args.batch
            return {k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in b.items()}
        prepare = lambda raws: ingest.text(raws, tok, 3000, "llava_v1")   # noqa: E731
        pfs = {k: Prefetcher(datasets[k].raw_item, 0, args.batch, prepare=prepare) for k in names if k.startswith("device")}

        def device_batch(name):
            raws, text = pfs[name].get()
            for r in raws:
                a = r.get("aug")
                if a is not None and name == "device_aug":
                    seen["samples"] += 1
                    seen["flip"] += a["flip"]
                    seen["jitter"] += a["jitter"] is not None
                if "crop" in r:
                    seen["crop_samples"] += 1
                    seen["crop"] += r["crop"] is not None
            return ingest.batch(raws, tok, 3000, "llava_v1", text=text)
        feeds = {k: (lambda k=k: device_batch(k)) if k.startswith("device") else (lambda k=k: host_batch(k)) for k in names}
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
            for pf in pfs.values():
                pf.close()
        med = {k: statistics.median(v) for k, v in sps.items()}
        result["sizes"][size] = {
            "samples_per_s": {k: [round(x, 2) for x in v] for k, v in sps.items()},
            "samples_per_s_median": {k: round(v, 2) for k, v in med.items()},
            "main_thread_ms_per_step_getting_the_batch": {k: [round(x, 1) for x in v] for k, v in data_ms.items()},
            "device_aug_samples_flipped_jittered_of": [seen["flip"], seen["jitter"], seen["samples"]],
            "host_augments": ingest.host_augments, "host_fills": ingest.host_fills}
        if "device_crop" in feeds:
            result["sizes"][size].update({"device_crop_samples_cropped_of": [seen["crop"], seen["crop_samples"]],
                                          "host_crops": ingest.host_crops, "crop_skipped": ingest.crop_skipped})
        if {"device_crop", "host_crop", "device_aug", "host_aug", "device"} <= set(feeds):
            result["sizes"][size].update({
                "device_crop_over_device_aug": round(med["device_crop"] / med["device_aug"], 3),
                "device_crop_inside_the_plain_device_feeds_spread": bool(min(sps["device"]) <= med["device_crop"] <= max(sps["device"])),
                "host_crop_over_host_aug": round(med["host_crop"] / med["host_aug"], 3)})
        if {"device", "device_aug", "host_aug"} <= set(feeds):
            result["sizes"][size].update({
                "device_aug_over_device": round(med["device_aug"] / med["device"], 3),
                "device_aug_inside_the_plain_device_feeds_spread": bool(min(sps["device"]) <= med["device_aug"] <= max(sps["device"])),
                "host_aug_over_device_aug": round(med["host_aug"] / med["device_aug"], 3)})
    result["loss_first_last"] = [round(float(losses[0]), 4), round(float(losses[-1]), 4)]
    result["peak_hbm_gb"] = round(torch.cuda.max_memory_allocated() / 2 ** 30, 1)
    print(json.dumps(result))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
