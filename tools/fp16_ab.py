#!/usr/bin/env python3
"""fp16 vs bf16 inference mode, one process, alternating (bench.py's workload: BASELINE.json configs[2] by default — 7B, 64 x 1024^2
frames, 32-token prompt, 8 generated tokens; the same bf16 weight VALUES for both models, bench.py's inputs, warm-up and timing fence).

  python tools/fp16_ab.py [--config 7b] [--batch 64] [--rounds 3] [--steps 5] [--warmup 2] [--b1]

Prints one JSON line: frames/s of each mode per round and their medians, the fp16 / bf16 ratio, (--b1) the batch-1 frame latency and
(--parity) full_frame_parity(): one full-depth frame of both modes against the CPU oracle. bench.py itself times bf16 only."""
import argparse
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from haff import config as hcfg  # noqa: E402
from haff import dist as hdist  # noqa: E402
from haff import weights as hw  # noqa: E402
from haff.lisa import LisaMI355  # noqa: E402


def _exact_in_all(t):
    """bf16 values with |v| < 2^-14 zeroed: exact in bf16, fp16 (normal range) and fp32 alike."""
    t = t.to(torch.bfloat16)
    return t.masked_fill_(t.abs() < 2.0 ** -14, 0)


def full_frame_parity(cfg, device, threads, text_tokens=32, n_gen=8, seed=1234):
    """One full-depth frame (bench.py's Gaussian field: its noise frame, prompt and forced answer with one [SEG]) through
    LisaMI355.evaluate in bf16 and fp16 and through oracle.lisa_evaluate on ONE weight set that all three represent exactly. Returns
    per mode: token ids equal, IoU left / right, max |logit err| / scale, taxonomy error, max |x| of the ViT-H residual stream,
    finiteness; or {"skipped": why} when the host cannot hold the oracle's fp32 copy of the weights."""
    from oracle import lisa_oracle as O
    n_par = sum(math.prod(v) for v in hw.all_shapes(cfg).values())
    try:
        import psutil
        need = n_par * 4 * 1.25 + 8e9
        if psutil.virtual_memory().available < need:
            return {"skipped": "host memory: %.0f GB available, %.0f GB needed for the oracle's fp32 copy of the weights" %
                               (psutil.virtual_memory().available / 1e9, need / 1e9)}
    except ImportError:
        pass
    torch.set_num_threads(threads)
    S = cfg.sam.img_size
    sizes = [(S, S)]
    sd_dev = hw.make_state_dict_device(cfg, seed, device, torch.bfloat16)
    for k in sd_dev:
        sd_dev[k] = _exact_in_all(sd_dev[k])
    frames, images_clip, ids, forced = bench.make_inputs(cfg, 1, text_tokens, n_gen, device, seed=seed)
    images = _exact_in_all(O.sam_preprocess(frames[0].cpu().numpy(), S)[None]).float()
    clip = _exact_in_all(images_clip.cpu()).float()
    sd = {k: v.cpu().float() for k, v in sd_dev.items()}
    with torch.no_grad():
        r_ids, r_left, r_right, r_tax = O.lisa_evaluate(sd, cfg, clip, images, ids.cpu(), sizes, sizes, max_new_tokens=n_gen,
                                                        forced_answer=forced.cpu(), use_cache=True)
    del sd
    res = {}
    for name, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        model = LisaMI355(cfg, sd_dev, dtype=dt, device=device)
        o_ids, left, right, tax = model.evaluate(clip.to(device), images.to(device), ids, sizes, sizes, max_new_tokens=n_gen,
                                                 forced_answer=forced)
        taps = {}
        model.sam_encoder(images.to(device), taps)
        torch.cuda.synchronize()
        row = {"token_ids_equal": bool(torch.equal(o_ids.cpu(), r_ids)),
               "vit_stream_max_abs": max(v.abs().max().item() for v in taps.values()),
               "finite": bool(all(torch.isfinite(t).all() for t in (left[0], right[0], tax[0])))}
        errs = []
        for hand, got, ref in (("left", left[0], r_left[0]), ("right", right[0], r_right[0])):
            g = got.cpu()
            a, b = g > 0, ref > 0
            union = (a | b).sum().item()
            row["iou_" + hand] = round((a & b).sum().item() / union if union else 1.0, 6)
            errs.append((g - ref).abs().max().item() / ref.abs().max().item())
        row["logit_max_rel_err"] = max(errs)
        row["taxonomy_max_abs_err"] = (tax[0].cpu() - r_tax[0]).abs().max().item()
        res[name] = row
        del model, taps
        torch.cuda.empty_cache()
    return res


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="7b", choices=["7b", "13b", "tiny", "mid"])
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--text-tokens", type=int, default=32)
    ap.add_argument("--n-gen", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--b1", action="store_true", help="also the batch-1 frame latency of each mode")
    ap.add_argument("--parity", action="store_true", help="also one full-depth frame of both modes against the oracle")
    args = ap.parse_args(argv)
    device = torch.device("cuda:0")
    cfg = {"7b": hcfg.haff_7b, "13b": hcfg.haff_13b, "tiny": hcfg.tiny, "mid": hcfg.mid}[args.config]()
    sd = hw.make_state_dict_device(cfg, 1234, device, torch.bfloat16)
    models = {"bf16": LisaMI355(cfg, sd, dtype=torch.bfloat16, device=device, sam_chunk="auto"),   # bench.py's default configuration
              "fp16": LisaMI355(cfg, sd, dtype=torch.float16, device=device, sam_chunk="auto")}
    del sd
    torch.cuda.empty_cache()
    B, S = args.batch, cfg.sam.img_size
    frames, _, ids, forced = bench.make_inputs(cfg, B, args.text_tokens, args.n_gen, device, seed=1234)
    sizes = [(S, S)] * B

    def step(model, n=B):
        return model.evaluate(None, None, ids[:n], sizes[:n], sizes[:n], max_new_tokens=args.n_gen, forced_answer=forced[:n],
                              frames_u8=frames[:n])

    for m in models.values():
        for _ in range(args.warmup):
            step(m)
    fps = {k: [] for k in models}
    for _ in range(args.rounds):
        for name, m in models.items():
            elapsed = hdist.timed_steps(lambda: step(m), args.steps, device)
            fps[name].append(B * args.steps / elapsed)
    res = {"config": args.config, "batch": B, "steps": args.steps, "rounds": args.rounds,
           "fps": {k: [round(v, 2) for v in vs] for k, vs in fps.items()},
           "fps_median": {k: round(statistics.median(vs), 2) for k, vs in fps.items()}}
    res["fp16_over_bf16"] = round(res["fps_median"]["fp16"] / res["fps_median"]["bf16"], 4)
    if args.b1:
        lat = {}
        for name, m in models.items():
            step(m, 1)
            elapsed = hdist.timed_steps(lambda: step(m, 1), max(args.steps, 5), device)
            lat[name] = round(1e3 * elapsed / max(args.steps, 5), 2)
        res["b1_ms"] = lat
    if args.parity:
        del models
        torch.cuda.empty_cache()
        res["parity"] = full_frame_parity(cfg, device, min(len(os.sched_getaffinity(0)), 32), args.text_tokens, args.n_gen)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
