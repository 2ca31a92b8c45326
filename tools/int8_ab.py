#!/usr/bin/env python3
"""fp16 vs fp16 + LLM.int8 weights (load_in_8bit=True) vs fp16 + NF4 (load_in_4bit=True), one process, alternating, on the same weight
values (bench.py's inputs, warm-up and timing fence; the weights are drawn once and quantised on load by the quantised models).

  python tools/int8_ab.py [--config 7b] [--batch 8] [--rounds 3] [--steps 5] [--warmup 2] [--b1] [--b8-step] [--only int8,fp16]
  python tools/int8_ab.py --kernel-report <rocprofv3 kernel_trace.csv> [--config 7b]

Prints one JSON line: frames/s of each mode per round and their medians, the ratios to fp16, the Llama + lm_head bytes, and (--b1)
per mode the batch-1 frame latency with its split: the decode step (the difference of an 8-token and a 3-token reply, over 5 steps)
and the rest (prefill, encoders, decoder tail); --b8-step: the same split of the 8-frame step's decode step. --kernel-report reads a
`rocprofv3 --kernel-trace` CSV of a run of this tool and gives, per int8 product shape of the weight-streaming form, the dispatches,
median time and the achieved bytes/s of the int8 weight bytes (codes + fp32 row scales; activations and outputs not counted), and the
summed time of the tiled form and of the activation quantiser kernels."""
import argparse
import csv
import json
import os
import re
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _cfg(name):
    from haff import config as hcfg
    return {"7b": hcfg.haff_7b, "13b": hcfg.haff_13b, "tiny": hcfg.tiny, "mid": hcfg.mid}[name]()


def int8_shapes(cfg):
    """(N, K, swiglu) of every int8 product of a decode step -> name"""
    l = cfg.llm
    return {(3 * l.hidden, l.hidden, False): "qkv", (l.hidden, l.hidden, False): "o_proj", (2 * l.ffn, l.hidden, True): "gate_up",
            (l.hidden, l.ffn, False): "down_proj", (l.vocab, l.hidden, False): "lm_head"}


def kernel_report(path, cfg):
    """Per-shape int8 product times from a rocprofv3 kernel trace. A gemm_i8_skinny_kernel<MT, NT, SWIGLU, KW> workgroup covers
    16 * NT weight rows, so (SWIGLU, workgroups, NT) identifies N."""
    shapes = int8_shapes(cfg)
    rows, other = {}, {}
    with open(path) as fh:
        for r in csv.DictReader(fh):
            kn = r.get("Kernel_Name", "")
            dur = int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
            for k in ("i8_act_row_kernel", "i8_act_scan_kernel", "i8_act_codes_kernel", "i8_act_cols_kernel", "gemm_i8_tiled_kernel",
                      "i8_weight_kernel"):
                if k in kn:
                    o = other.setdefault(k, [0, 0])
                    o[0] += 1
                    o[1] += dur
            m = re.search(r"gemm_i8_skinny_kernel<(\d+), (\d+), (true|false), (\d+)>", kn)
            if not m:
                continue
            nt, sw = int(m.group(2)), m.group(3) == "true"
            wg = int(r["Grid_Size_X"]) // int(r["Workgroup_Size_X"])
            hits = [(N, K, name) for (N, K, s), name in shapes.items() if s == sw and (N + 16 * nt - 1) // (16 * nt) == wg]
            if hits:   # shapes with the same grid (7B: o_proj and down_proj) are one entry; bytes: their mean
                key = "+".join(h[2] for h in hits)
                rows.setdefault(key, {"N": hits[0][0], "K": [h[1] for h in hits], "ns": []})["ns"].append(dur)
    out = {}
    for name, v in rows.items():
        nbytes = sum(v["N"] * k + 4 * v["N"] for k in v["K"]) // len(v["K"])
        med = statistics.median(v["ns"])
        out[name] = {"N": v["N"], "K": v["K"], "dispatches": len(v["ns"]), "median_us": round(med / 1e3, 2),
                     "int8_bytes": nbytes, "TBps": round(nbytes / med / 1e3, 3)}
    return {"int8_skinny_gemm": out,
            "other_kernels": {k: {"dispatches": n, "total_ms": round(ns / 1e6, 3), "mean_us": round(ns / n / 1e3, 2)}
                              for k, (n, ns) in other.items()}}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="7b", choices=["7b", "13b", "tiny", "mid"])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--text-tokens", type=int, default=32)
    ap.add_argument("--n-gen", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--b1", action="store_true", help="also the batch-1 frame latency and its decode-step split")
    ap.add_argument("--b8-step", action="store_true", help="also the decode step of the --batch frame step")
    ap.add_argument("--only", default="fp16,int8,nf4", help="comma list of the modes to build (profiling runs: one)")
    ap.add_argument("--kernel-report", help="rocprofv3 kernel trace CSV to summarise (no GPU work)")
    args = ap.parse_args(argv)
    cfg = _cfg(args.config)
    if args.kernel_report:
        print(json.dumps({"config": args.config, **kernel_report(args.kernel_report, cfg)}))
        return
    import torch
    import bench
    from haff import dist as hdist
    from haff import weights as hw
    from haff.lisa import LisaMI355
    device = torch.device("cuda:0")
    assert args.n_gen >= 3
    sd = hw.make_state_dict_device(cfg, 1234, device, torch.float16)
    models = {}
    for name in args.only.split(","):
        assert name in ("fp16", "int8", "nf4"), name
        models[name] = LisaMI355(cfg, sd, dtype=torch.float16, device=device, sam_chunk="auto", load_in_4bit=name == "nf4",
                                 load_in_8bit=name == "int8")
    del sd
    torch.cuda.empty_cache()
    B, S = args.batch, cfg.sam.img_size
    frames, _, ids, forced = bench.make_inputs(cfg, B, args.text_tokens, args.n_gen, device, seed=1234)
    sizes = [(S, S)] * B

    def step(model, n=B, n_gen=args.n_gen):
        f = forced[:n, :n_gen]
        return model.evaluate(None, None, ids[:n], sizes[:n], sizes[:n], max_new_tokens=n_gen, forced_answer=f, frames_u8=frames[:n])

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
           "fps_median": {k: round(statistics.median(vs), 2) for k, vs in fps.items()},
           "llm_weight_GB": {k: round(m.llm_weight_bytes() / 1e9, 3) for k, m in models.items()}}
    if "fp16" in models:
        for k in models:
            if k != "fp16":
                res[f"{k}_over_fp16"] = round(res["fps_median"][k] / res["fps_median"]["fp16"], 4)

    def split(nb):
        lat = {}
        n = max(args.steps, 10) if nb == 1 else args.steps
        for name, m in models.items():
            t = {}
            for g in (args.n_gen, 3):   # [SEG] is the third forced token either way: the same mask-decoder work
                step(m, nb, g)
                t[g] = 1e3 * hdist.timed_steps(lambda: step(m, nb, g), n, device) / n
            dstep = (t[args.n_gen] - t[3]) / (args.n_gen - 3)
            lat[name] = {"frame_ms" if nb == 1 else "step_ms": round(t[args.n_gen], 3), "decode_step_ms": round(dstep, 3),
                         "rest_ms": round(t[args.n_gen] - (args.n_gen - 1) * dstep, 3)}
        return lat
    if args.b1:
        res["b1"] = split(1)
    if args.b8_step:
        res[f"b{B}_step"] = split(B)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
