#!/usr/bin/env python3
"""What --smooth_masks costs, and what it replaces, on one MI355X (modelled on tools/score_ab.py, whose tree and helpers it uses):

  plain   : inference.py --score_only                                   (the yardstick: the same command without the flag)
  smooth  : inference.py --score_only --smooth_masks                    (haff_mask_quantile7 once per batch, then the same scorer)
  files   : inference.py (PNG planes per threshold), smooth.py over the written tree, evaluation.py --map   (the route the flag
            replaces: the reference's three-step workflow, with this repository's host tools)

on a generated ActAffordance-shaped tree, a synthetic model (--model, default 7b) with a forced [SEG] answer. The routes alternate,
each run a fresh child process under its own time limit; a run that fails or times out ends the job. The Hausdorff distances are
left out of every route, as in tools/score_ab.py.

And the kernel alone: haff_mask_quantile7 on two 855 x 855 and on two 1024 x 1024 planes, timed with device events after a warm-up,
against its traffic floor of 8 B per pixel (one read, one write) at the measured HBM copy rate.

  python tools/smooth_ab.py --frames 48 --reps 2 --out profiles/smooth_ab.json
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import score_ab   # noqa: E402  (make_tree, _Clock, _force_seg)

HBM_COPY_BYTES_PER_S = 6.29e12    # float4 copy, measured; the spec peak is 8.0e12
ROUTES = ("plain", "smooth", "files")


def worker_route(route, bench, work, batch, model):
    import contextlib
    import io
    import torch
    import haff  # noqa: F401
    from haff import evaluation, inference, postprocess, smooth
    score_ab._force_seg()
    clock = score_ab._Clock()
    clock.wrap(inference, "build_model_and_tokenizer", "model_build_s")
    clock.wrap(inference, "load_rgb", "frame_decode_s")
    argv = ["--synthetic", model, "--benchmark-dir", bench, "--vis_save_path", os.path.join(work, "th"), "--batch-size", str(batch)]
    if model == "tiny":
        argv += ["--image_size", "224"]
    sink = io.StringIO()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(sink):
        if route == "files":
            clock.wrap(inference, "save_mask", "png_encode_s")
            evaluation.calculate_hausdorff = lambda a, b: (0.0, 0.0)
            inference.main(argv)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            smooth.main(["--input_dir", work])
            clock.t["smooth_py_s"] = time.perf_counter() - t1
            t1 = time.perf_counter()
            res = evaluation.main(["--benchmark_folder", bench, "--comparison_folder", work, "--map"])
            clock.t["evaluation_s"] = time.perf_counter() - t1
        else:
            clock.wrap(postprocess, "smooth_mask_lists", "smooth_enqueue_s")
            res = inference.main(argv + ["--score_only"] + (["--smooth_masks"] if route == "smooth" else []))
            torch.cuda.synchronize()
    total = time.perf_counter() - t0
    out = {"route": route, "total_s": total, "route_s": total - clock.t["model_build_s"], "stages": clock.t,
           "count": res["best"]["count"], "mean_average_precision": res["mean_average_precision"],
           "best": {k: res["best"][k] for k in ("threshold", "iou", "iocm")}}
    print("__RESULT__" + json.dumps(out))


def worker_kernel(iters):
    import torch
    import haff  # noqa: F401
    from haff import ops
    dev = torch.device("cuda", 0)
    rows = []
    for side in (855, 1024):
        g = torch.Generator(device=dev).manual_seed(side)
        x = torch.randn((2, side, side), device=dev, generator=g) * 4
        for _ in range(5):
            ops.mask_quantile7(x, 32768)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
        ev[0].record()
        for i in range(iters):
            ops.mask_quantile7(x, 32768)       # allocates its output, as the CLI's call does
            ev[i + 1].record()
        torch.cuda.synchronize()
        ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(iters))
        floor_ms = 8.0 * x.numel() / HBM_COPY_BYTES_PER_S * 1e3
        rows.append({"planes": 2, "side": side, "iters": iters, "median_ms": ms[iters // 2], "min_ms": ms[0], "max_ms": ms[-1],
                     "traffic_floor_ms": floor_ms, "times_the_floor": ms[iters // 2] / floor_ms,
                     "pixels_per_s": x.numel() / (ms[iters // 2] * 1e-3)})
    print("__RESULT__" + json.dumps({"kernel": "haff_mask_quantile7, need 32768, Gaussian logits (the cost does not depend on the data)",
                                     "floor": "8 B per pixel at 6.29 TB/s (measured float4 copy)", "rows": rows}))


def _child(argv, limit):
    """One GPU-using step: a fresh process of this file under its own time limit. Returns its result dict, or raises."""
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, capture_output=True, text=True, timeout=limit, cwd=ROOT)
    if p.returncode != 0:
        raise RuntimeError(f"{argv}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("__RESULT__")][-1]
    return json.loads(line[len("__RESULT__"):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=48)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--model", default="7b", choices=["tiny", "mid", "7b", "13b"])
    ap.add_argument("--routes", nargs="+", default=list(ROUTES), choices=ROUTES)
    ap.add_argument("--kernel_iters", type=int, default=200)
    ap.add_argument("--limit", type=int, default=300, help="time limit of each child process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "smooth_ab.json"))
    ap.add_argument("--worker", default=None)
    ap.add_argument("--bench", default=None)
    ap.add_argument("--work", default=None)
    a = ap.parse_args()
    if a.worker in ROUTES:
        return worker_route(a.worker, a.bench, a.work, a.batch, a.model)
    if a.worker == "kernel":
        return worker_kernel(a.kernel_iters)
    kernel = _child(["--worker", "kernel", "--kernel_iters", str(a.kernel_iters)], a.limit)
    print(json.dumps(kernel), flush=True)
    with tempfile.TemporaryDirectory() as tmp:
        bench = os.path.join(tmp, "bench")
        score_ab.make_tree(bench, a.frames)
        runs = []
        for rep in range(a.reps):
            for route in a.routes:
                work = os.path.join(tmp, f"{route}{rep}")
                os.makedirs(work)
                runs.append(_child(["--worker", route, "--bench", bench, "--work", work, "--batch", str(a.batch),
                                             "--model", a.model], a.limit))
                print(json.dumps(runs[-1]), flush=True)
    fps = {r: [a.frames / x["route_s"] for x in runs if x["route"] == r] for r in a.routes}
    out = {"what": "cost of inference.py --smooth_masks and of the files route it replaces, one MI355X, synthetic model, forced "
                   "[SEG]; see tools/smooth_ab.py",
           "model": a.model, "frames": a.frames, "batch": a.batch, "reps": a.reps, "frames_per_s": fps, "kernel_alone": kernel,
           "runs": runs,
           "not_measured": ["Hausdorff distances (left out of every route)", "real ActAffordance frames", "more than one GPU"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"frames_per_s": fps, "kernel_alone": kernel["rows"]}))


if __name__ == "__main__":
    main()
