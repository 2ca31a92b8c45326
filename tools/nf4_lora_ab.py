#!/usr/bin/env python3
"""Plain NF4 vs NF4 + unmerged LoRA adapters (q,v and all seven projections), one process, alternating, on the same weights
(bench.py's inputs, warm-up and timing fence; modelled on tools/nf4_ab.py).

  python tools/nf4_lora_ab.py [--config 7b] [--rounds 3] [--steps 5] [--warmup 2] [--out profiles/nf4_lora_ab_7b.json]

Prints (and with --out writes) one JSON object:
  models   per mode and round: frames/s at --batch frames, the batch-1 frame, and the decode step at 1 and at --batch rows (the
           difference of an 8-token and a 3-token reply over 5 steps, as nf4_ab.py splits it), with medians; the spread between
           the plain mode's own rounds; the adapters' bytes.
  t_launch the event-timed t = x A_cat^T launch (ops.linear, [M, 4096] x [24, 4096]) at 1 and 8 rows.
  kernels  event-timed, at the four projection shapes: haff_nf4_dequant_f16 against haff_nf4_dequant_lora_f16, and haff_gemm_nf4_f16
           against haff_gemm_nf4_lora_f16 (t given) at 1 and 8 rows; us per launch and TB/s of the bytes the kernel must move (codes +
           absmax, and for the dequantisation the f16 output), over enough distinct copies of the weight that no launch finds its
           codes in the 256 MB last-level cache.
  checks   the two margins of the issue: the q,v decode step against plain + 32 t launches + the plain spread, and kernel 1
           against the plain dequantisation on the same shapes.
The plain mode keeps lm_head in f16 (nf4_lm_head=False), as the adapter modes do (the trainer's quantised set)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALL7 = "q_proj,k_proj,v_proj,o_proj,gate_proj,up_proj,down_proj"


def _cfg(name):
    from haff import config as hcfg
    return {"7b": hcfg.haff_7b, "13b": hcfg.haff_13b, "tiny": hcfg.tiny, "mid": hcfg.mid}[name]()


def _event_us(fn, n, torch):
    """us per call of fn(i), i = 0..n-1, between two device events (one warm-up pass first)."""
    for i in range(min(n, 8)):
        fn(i)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(n):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return 1e3 * a.elapsed_time(b) / n


def kernel_times(cfg, device, torch, rows=(1, 8), n=200):
    import math
    from haff import ops, quant
    H, F = cfg.llm.hidden, cfg.llm.ffn
    shapes = {"qkv": (3 * H, H, 3, H, False), "o_proj": (H, H, 1, 16, False), "gate_up": (2 * F, H, 2, 16, True),
              "down_proj": (H, F, 1, 16, False)}
    g = torch.Generator(device=device).manual_seed(7)
    out = {}
    for name, (N, K, nseg, seg_rows, swiglu) in shapes.items():
        nbytes = N * K // 2 + N * (K // 64) * 4
        copies = max(2, -(-(640 << 20) // nbytes))          # > 2x the last-level cache in flight between two uses of a copy
        base = quant.quantize([(torch.randn(N, K, device=device, generator=g) * 0.02, None)], device)
        ws = [base] + [quant.Nf4Weight(base.packed.clone(), base.absmax.clone()) for _ in range(copies - 1)]
        a_cat = ((torch.rand((8 * nseg, K), device=device, generator=g) * 2 - 1) / math.sqrt(K)).half()
        b = ((torch.rand((N, 8), device=device, generator=g) * 2 - 1) * 0.05).half()
        L = quant.Nf4Lora(a_cat, b, nseg, seg_rows, 2.0)
        scratch = torch.empty((N, K), dtype=torch.float16, device=device)
        rec = {"N": N, "K": K, "nf4_bytes": nbytes, "copies": copies}
        for key, fn in (("dequant", lambda i: ops.nf4_dequant(ws[i % copies].packed, ws[i % copies].absmax, out=scratch)),
                        ("dequant_lora", lambda i: ops.nf4_dequant_lora(ws[i % copies].packed, ws[i % copies].absmax, L, out=scratch))):
            us = _event_us(fn, n, torch)
            rec[key] = {"us": round(us, 2), "TBps": round((nbytes + 2 * N * K) / us / 1e6, 3)}
        rec["dequant_lora_over_plain"] = round(rec["dequant_lora"]["us"] / rec["dequant"]["us"], 4)
        for M in rows:
            x = torch.randn(M, K, device=device, generator=g).half()
            t = ops.linear(x, a_cat)
            y = torch.empty((M, N // 2 if swiglu else N), dtype=torch.float16, device=device)
            for key, fn in ((f"gemm_m{M}", lambda i: ops.linear_nf4(x, ws[i % copies].packed, ws[i % copies].absmax, swiglu=swiglu, out=y)),
                            (f"gemm_lora_m{M}", lambda i: ops.linear_nf4(x, ws[i % copies].packed, ws[i % copies].absmax, swiglu=swiglu,
                                                                         out=y, lora=L, lora_t=t))):
                us = _event_us(fn, n, torch)
                rec[key] = {"us": round(us, 2), "TBps": round(nbytes / us / 1e6, 3)}
        out[name] = rec
        del ws
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="7b", choices=["7b", "13b", "tiny", "mid"])
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--text-tokens", type=int, default=32)
    ap.add_argument("--n-gen", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--skip-kernels", action="store_true")
    ap.add_argument("--out", help="also write the JSON object to this file")
    args = ap.parse_args(argv)
    cfg = _cfg(args.config)
    import torch
    import bench
    from haff import dist as hdist
    from haff import ops
    from haff import train_model as TM
    from haff import weights as hw
    from haff.lisa import LisaMI355
    device = torch.device("cuda:0")
    assert args.n_gen >= 4
    sd = hw.make_state_dict_device(cfg, 1234, device, torch.float16)
    models = {}
    for name, targets in (("nf4", None), ("nf4_lora_qv", "q_proj,v_proj"), ("nf4_lora_all7", ALL7)):
        kw = {"nf4_lm_head": False}
        if targets:
            kw = {"lora_state": TM.init_lora(cfg, TM.lora_targets(cfg, targets), 8, 0, init_b_zero=False), "lora_alpha": 16}
        models[name] = LisaMI355(cfg, sd, dtype=torch.float16, device=device, sam_chunk="auto", load_in_4bit=True, **kw)
    del sd
    torch.cuda.empty_cache()
    B, S = args.batch, cfg.sam.img_size
    frames, _, ids, forced = bench.make_inputs(cfg, B, args.text_tokens, args.n_gen, device, seed=1234)
    sizes = [(S, S)] * B

    def step(model, n=B, n_gen=args.n_gen):
        return model.evaluate(None, None, ids[:n], sizes[:n], sizes[:n], max_new_tokens=n_gen, forced_answer=forced[:n, :n_gen],
                              frames_u8=frames[:n])

    for m in models.values():
        for n in (B, 1):
            for g in (args.n_gen, 3):
                for _ in range(args.warmup):
                    step(m, n, g)
    keys = ("fps", "frame_ms_b1", "decode_step_ms_b1", f"decode_step_ms_b{B}")
    per = {name: {k: [] for k in keys} for name in models}
    nb1 = max(args.steps, 10)
    for _ in range(args.rounds):
        for name, m in models.items():
            t = {}
            for n, reps in ((B, args.steps), (1, nb1)):
                for g in (args.n_gen, 3):   # [SEG] is the third forced token either way: the same mask-decoder work
                    t[n, g] = 1e3 * hdist.timed_steps(lambda: step(m, n, g), reps, device) / reps
            per[name]["fps"].append(B * 1e3 / t[B, args.n_gen])
            per[name]["frame_ms_b1"].append(t[1, args.n_gen])
            per[name]["decode_step_ms_b1"].append((t[1, args.n_gen] - t[1, 3]) / (args.n_gen - 3))
            per[name][f"decode_step_ms_b{B}"].append((t[B, args.n_gen] - t[B, 3]) / (args.n_gen - 3))
    res = {"config": args.config, "batch": B, "steps": args.steps, "rounds": args.rounds, "models": {}}
    for name, m in models.items():
        res["models"][name] = {k: {"rounds": [round(v, 4) for v in vs], "median": round(statistics.median(vs), 4)}
                               for k, vs in per[name].items()}
        res["models"][name]["llm_weight_GB"] = round(m.llm_weight_bytes() / 1e9, 3)
        res["models"][name]["lora_MB_per_layer"] = round(m.llm.lora_bytes() / 1e6 / len(m.llm.layers), 3)
    spread = {k: round(max(per["nf4"][k]) - min(per["nf4"][k]), 4) for k in keys}
    res["plain_spread"] = spread
    H = cfg.llm.hidden
    a_cat = torch.randn((24, H), device=device).half()
    res["t_launch_us"] = {}
    for M in (1, B):
        x = torch.randn((M, H), device=device).half()
        res["t_launch_us"][f"m{M}"] = round(_event_us(lambda i: ops.linear(x, a_cat), 500, torch), 2)
    med = lambda name, k: res["models"][name][k]["median"]   # noqa: E731
    checks = {}
    for M in (1, B):
        k = f"decode_step_ms_b{M}"
        allowed = med("nf4", k) + 32 * res["t_launch_us"][f"m{M}"] / 1e3 + spread[k]
        checks[f"qv_{k}"] = {"plain": med("nf4", k), "qv": med("nf4_lora_qv", k), "allowed": round(allowed, 4),
                             "within": med("nf4_lora_qv", k) <= allowed}
    if not args.skip_kernels:
        del models
        torch.cuda.empty_cache()
        res["kernels"] = kernel_times(cfg, device, torch, rows=(1, B))
        checks["dequant_lora_over_plain"] = {n: r["dequant_lora_over_plain"] for n, r in res["kernels"].items()}
    res["checks"] = checks
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
