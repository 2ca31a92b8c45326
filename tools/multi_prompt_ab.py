#!/usr/bin/env python3
"""A/B of several prompts on one frame, on one MI355X: LisaMI355.evaluate(offset=) — encoders once per frame, the prompts' common
prefix prefilled once per frame and broadcast (haff_kv_prefix_broadcast) — against the same rows each carrying its own copy of the
frame through the plain call (offset=None).

  python tools/multi_prompt_ab.py --model 7b --out profiles/multi_prompt_ab_7b.json

Synthetic weights, bf16, 1024^2 uint8 frames (frames_u8: both towers' inputs are made on the device). The prompt has the shape of the
CLIs' inference prompt: BOS <im_start> <image> <im_end> + 17 ids of the question that every row shares + 8 ids of the row's own action;
8 forced tokens with one [SEG]. Points: F = 1 frame with N = 1, 2, 4, 8 prompts, and F = 8 frames with N = 4 prompts each. At every
point both routes are warmed up (two calls each: the first call of a shape runs its decode step eagerly and captures it), then
alternate (the one that goes first too) for --rounds rounds of --iters calls, each round timed with a host clock between device synchronisations. Recorded per point:
ms per call of both routes for every round, last_group_plan, the broadcast kernel's event-timed time per layer on the call's own
caches with the bytes it moved, and the largest difference between the two routes' results. A run without a GPU fails.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_WRITE_BPS = 6.3e12          # achievable HBM bandwidth of the MI355X (float4 copy: 6.29 TB/s measured of 8 TB/s)
SHARED_IDS, ACTION_IDS, N_GEN = 17, 8, 8
POINTS = ((1, 1), (1, 2), (1, 4), (1, 8), (8, 4))


def make_point(cfg, F, N, device, seed=1234):
    import torch
    g = torch.Generator(device="cpu").manual_seed(seed)
    S = cfg.sam.img_size
    noise = torch.randint(0, 256, (F, S, S, 3), generator=g, dtype=torch.int32).float()
    yy = torch.linspace(0, 255, S).view(1, S, 1, 1)
    xx = torch.linspace(255, 0, S).view(1, 1, S, 1)
    frames = (0.5 * noise + 0.25 * yy + 0.25 * xx).round().clamp(0, 255).to(torch.uint8)
    hi = min(cfg.llm.vocab, cfg.seg_token_idx) - 1
    B = F * N
    head = torch.tensor([cfg.bos_token_id, cfg.im_start_idx, -200, cfg.im_end_idx])
    shared = torch.randint(3, hi, (SHARED_IDS,), generator=g)
    actions = torch.randint(3, hi, (B, ACTION_IDS), generator=g)
    ids = torch.cat([torch.cat([head, shared])[None].expand(B, -1), actions], 1).long()
    forced = torch.randint(3, hi, (B, N_GEN), generator=g).long()
    forced[:, 2] = cfg.seg_token_idx
    forced[:, -1] = cfg.eos_token_id
    offset = torch.arange(F + 1, dtype=torch.int64) * N
    frame_of = torch.arange(F).repeat_interleave(N)
    return frames.to(device), ids.to(device), forced.to(device), offset, frame_of


def time_broadcast(model, F, B, reps=7):
    """The broadcast of the last grouped call again, on that call's caches: all layers back to back between two events."""
    import torch
    from haff import ops
    plan = model.last_group_plan
    Pp = plan["prefix_positions"]
    pre = model._prefix_caches[(F, Pp)]
    cache = next(c for (b, _), c in model._caches.items() if b == B)
    frame_of = torch.arange(F, dtype=torch.int32).repeat_interleave(B // F).to(model.device)
    layers = len(model.llm.layers)
    us = []
    for _ in range(reps + 2):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for li in range(layers):
            ops.kv_prefix_broadcast(pre["k"][li], pre["v"][li], cache["k"][li], cache["v"][li], frame_of, Pp)
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / layers)
    us = us[2:]
    elem = pre["k"][0].element_size()
    written = 2 * B * Pp * model.cfg.llm.hidden * elem
    bound_us = written / HBM_WRITE_BPS * 1e6
    med = statistics.median(us)
    return {"us_per_layer": us, "us_per_layer_median": med, "layers": layers, "bytes_written_per_layer": written,
            "bytes_read_per_layer": written, "hbm_write_bound_us": bound_us, "share_of_bound": bound_us / med,
            "written_TBps": written / med / 1e6}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", default="7b", choices=["tiny", "mid", "7b", "13b"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--iters", type=int, default=8, help="evaluate() calls per timed round and route")
    ap.add_argument("--points", default=None, help="F:N,F:N,... (default: 1:1,1:2,1:4,1:8,8:4)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multi_prompt_ab_7b.json"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("multi_prompt_ab.py measures on the MI355X: no GPU here, nothing measured")
    import haff  # noqa: F401
    from haff import checkpoint, config as hcfg
    from haff.lisa import LisaMI355
    device = torch.device("cuda", 0)
    cfg = {"tiny": hcfg.tiny, "mid": hcfg.mid, "7b": hcfg.haff_7b, "13b": hcfg.haff_13b}[a.model]()
    sd = checkpoint.synthetic_state_dict(cfg, 1234, device)
    model = LisaMI355(cfg, sd, dtype=torch.bfloat16, device=device)
    del sd
    S = cfg.sam.img_size
    points = POINTS if a.points is None else tuple(tuple(int(x) for x in p.split(":")) for p in a.points.split(","))
    results = []
    for F, N in points:
        B = F * N
        frames, ids, forced, offset, frame_of = make_point(cfg, F, N, device)
        copies = frames.index_select(0, frame_of.to(device)).contiguous()       # the ungrouped route's input: one copy per row

        def grouped():
            return model.evaluate(None, None, ids, [(S, S)] * F, [(S, S)] * F, max_new_tokens=N_GEN, forced_answer=forced,
                                  frames_u8=frames, offset=offset)

        def ungrouped():
            return model.evaluate(None, None, ids, [(S, S)] * B, [(S, S)] * B, max_new_tokens=N_GEN, forced_answer=forced,
                                  frames_u8=copies)
        outs = {}
        for name, fn in (("ungrouped", ungrouped), ("grouped", grouped)):      # warm-up: both calls of every shape
            fn()
            outs[name] = fn()
            if name == "grouped":
                plan = dict(model.last_group_plan)
        torch.cuda.synchronize()
        ms = {"grouped": [], "ungrouped": []}
        for rnd in range(a.rounds):
            order = (("ungrouped", ungrouped), ("grouped", grouped))
            for name, fn in (order if rnd % 2 == 0 else order[::-1]):       # the route that goes first alternates too
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(a.iters):
                    fn()
                torch.cuda.synchronize()
                ms[name].append((time.perf_counter() - t0) * 1e3 / a.iters)
        go, uo = outs["grouped"], outs["ungrouped"]
        diff = {"ids_equal": bool(torch.equal(go[0], uo[0])),
                "mask_max_abs_diff": max(float((x - y).abs().max()) for side in (1, 2) for x, y in zip(go[side], uo[side]) if x.numel()),
                "mask_scale": max(float(y.abs().max()) for side in (1, 2) for y in uo[side] if y.numel())}
        point = {"frames": F, "prompts_per_frame": N, "rows": B, "ms_per_call": ms, "last_group_plan": plan,
                 "grouped_median_ms": statistics.median(ms["grouped"]), "ungrouped_median_ms": statistics.median(ms["ungrouped"]),
                 "ungrouped_spread_ms": max(ms["ungrouped"]) - min(ms["ungrouped"]), "results": diff}
        point["speedup"] = point["ungrouped_median_ms"] / point["grouped_median_ms"]
        if plan["shared"]:
            grouped()
            point["broadcast"] = time_broadcast(model, F, B)
        results.append(point)
        print(json.dumps(point), flush=True)
        del frames, copies
    one = {p["prompts_per_frame"]: p for p in results if p["frames"] == 1}
    extra = {str(n): (p["grouped_median_ms"] - one[1]["grouped_median_ms"]) / (n - 1) for n, p in one.items() if n > 1 and 1 in one}
    conditions = {}
    for p in results:
        key = f"F{p['frames']}xN{p['prompts_per_frame']}"
        lo, hi = min(p["ms_per_call"]["ungrouped"]), max(p["ms_per_call"]["ungrouped"])
        if p["prompts_per_frame"] == 1:
            conditions[key] = {"plain_path": p["last_group_plan"]["shared"] is False,
                               "grouped_inside_ungrouped_spread": bool(lo <= p["grouped_median_ms"] <= hi)}
        else:
            conditions[key] = {"grouped_faster_by_more_than_the_spread":
                               bool(p["ungrouped_median_ms"] - p["grouped_median_ms"] > p["ungrouped_spread_ms"])}
    out = {"what": "evaluate(offset=) against the same rows with one frame copy each (offset=None), one MI355X; tools/multi_prompt_ab.py",
           "model": a.model, "dtype": "bf16", "frame": [S, S], "prompt_ids": 4 + SHARED_IDS + ACTION_IDS, "new_tokens": N_GEN,
           "rounds": a.rounds, "calls_per_round": a.iters, "hbm_write_bandwidth_assumed_Bps": HBM_WRITE_BPS, "points": results,
           "extra_ms_per_further_prompt_on_a_frame": extra, "conditions": conditions,
           "not_measured": ["a trained checkpoint and its tokenizer (ids are random, the prompt's shape is the CLI's)", "fp16 / NF4 / int8 modes",
                            "more than one GPU"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"conditions": conditions, "extra_ms_per_further_prompt": extra,
                      "speedups": {f"F{p['frames']}xN{p['prompts_per_frame']}": round(p["speedup"], 3) for p in results}}))


if __name__ == "__main__":
    main()
