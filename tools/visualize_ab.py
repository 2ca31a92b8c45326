#!/usr/bin/env python3
"""What the overlay panels cost, end to end and on the device, on one MI355X:

  score_only : inference.py --score_only                                   (no panels)
  visualize  : inference.py --score_only --visualize D --visualize_examples 0   (every scored frame drawn by the scoring call)
  files      : inference.py (PNG planes per threshold), then evaluation.py --visualize over the 0.5 tree, every frame

on tools/score_ab.py's generated tree (256 x 256 frames, 855 x 855 masks), the tiny synthetic model with a forced [SEG] answer. The
routes alternate, each run a fresh child process under its own time limit; a run that fails or times out ends the job.

The overlay launch alone: haff_score_masks with and without overlay records on the same batch, between device events, the median
of the differences, beside the launch's floor of 3 B read + 6 B written per frame pixel at 6.29 TB/s (the launch also reads the
planes it decides from, which the floor leaves out).

--parent DIR: a built checkout of the parent commit (`git worktree add DIR HEAD~1`, then its build()). After the routes, plain
--score_only of this tree and of that checkout alternate --parent_reps times, this file's worker importing that checkout's package:
the block "score_only_vs_parent" of the output.

  python tools/visualize_ab.py --frames 100 --reps 2 [--parent DIR] --out profiles/visualize_ab.json
"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.environ.get("HAFF_AB_ROOT") or HERE       # a worker started for --parent imports that checkout's package
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(HERE, "tools"))

import score_ab  # noqa: E402

HBM_BYTES_PER_S = 6.29e12                           # the measured copy rate README and DESIGN.md use for every floor


def worker_route(route, bench, work, batch):
    import contextlib
    import io
    import torch
    import haff  # noqa: F401
    from haff import evaluation, inference, scoring
    score_ab._force_seg()
    clock = score_ab._Clock()
    clock.wrap(inference, "build_model_and_tokenizer", "model_build_s")
    clock.wrap(inference, "load_rgb", "frame_decode_s")
    if hasattr(evaluation, "write_panel"):     # absent in the --parent checkout
        clock.wrap(evaluation, "write_panel", "captions_and_png_s")
    argv = ["--synthetic", "tiny", "--benchmark-dir", bench, "--vis_save_path", os.path.join(work, "th"), "--image_size", "224",
            "--batch-size", str(batch)]
    panels = os.path.join(work, "panels")
    sink = io.StringIO()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(sink):
        if route == "files":
            clock.wrap(inference, "save_mask", "mask_png_encode_s")
            inference.main(argv)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            done = evaluation.main(["--benchmark_folder", bench, "--comparison_folder", os.path.join(work, "th0.5"), "--visualize",
                                    "--visualize-dir", panels, "--num-examples", "1000000"])
            clock.t["evaluation_s"] = time.perf_counter() - t1
            count = len(done)
        else:
            clock.wrap(scoring.BenchmarkScorer, "add_batch", "scorer_add_batch_s")
            extra = ["--visualize", panels, "--visualize_examples", "0"] if route == "visualize" else []
            count = inference.main(argv + ["--score_only"] + extra)["best"]["count"]
    total = time.perf_counter() - t0
    written = len(os.listdir(panels)) if os.path.isdir(panels) else 0
    print("__RESULT__" + json.dumps({"route": route, "total_s": total, "route_s": total - clock.t["model_build_s"], "stages": clock.t,
                                     "count": count, "panels": written}))


def worker_kernel(frame_hw, n_frames, reps):
    """haff_score_masks over n_frames frames of frame_hw against 855 x 855 masks from 256 x 256 logits, with and without overlays."""
    import numpy as np
    import torch
    import haff  # noqa: F401
    from haff import cvlite, ops, postprocess, scoring
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    hf, wf = frame_hw
    ths = [postprocess.sigmoid_logit_threshold(t) for t in postprocess.THRESHOLDS]
    row = torch.from_numpy(cvlite.nearest_indices(hf, 855).astype(np.int32)).to(dev)
    col = torch.from_numpy(cvlite.nearest_indices(wf, 855).astype(np.int32)).to(dev)
    frames, records = [], []
    for i in range(n_frames):
        f = {"target_hw": (855, 855), "taxonomy": torch.tensor([0.1, 0.1, 0.7, 0.1], device=dev)}
        for side in ("left", "right"):
            f[side] = torch.from_numpy(rng.standard_normal((256, 256)).astype(np.float32).cumsum(0).cumsum(1) / 64).to(dev)
            f[f"gt_{side}"] = torch.from_numpy((rng.random((855, 855)) < 0.3).astype(np.uint8) * 255).to(dev)
        canvas = torch.empty((hf, 2 * wf, 3), dtype=torch.uint8, device=dev)
        records.append({"rgb": torch.from_numpy(rng.integers(0, 256, (hf, wf, 3), dtype=np.uint8)).to(dev), "row": row, "col": col, "t": 2,
                        "out": (canvas[:, :wf], canvas[:, wf:])})
        frames.append(f)
    plain = scoring.pack_frames(frames)
    drawn = scoring.pack_frames([dict(f, vis=i + 1) for i, f in enumerate(frames)])
    vis = scoring.pack_vis(records)
    counts = torch.empty((n_frames, len(ths), 4), dtype=torch.int32, device=dev)

    def timed(table, v):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        ops.score_masks(table, ths, dev, out_counts=counts, vis=v)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) * 1e-3
    with_vis, without = [], []
    for rep in range(reps + 3):                # the first rounds warm both paths up and are not reported
        w, p = timed(drawn, vis), timed(plain, None)
        if rep >= 3:
            with_vis.append(w)
            without.append(p)
    diff = sorted(w - p for w, p in zip(with_vis, without))
    floor = 9.0 * hf * wf * n_frames / HBM_BYTES_PER_S
    print("__RESULT__" + json.dumps({
        "frame_hw": [hf, wf], "frames": n_frames, "reps": reps, "call_with_overlays_s": sorted(with_vis)[len(with_vis) // 2],
        "call_without_s": sorted(without)[len(without) // 2], "overlay_launch_s": diff[len(diff) // 2],
        "overlay_launch_spread_s": [diff[0], diff[-1]], "floor_s": floor, "floor_bytes": 9 * hf * wf * n_frames,
        "note": "each call includes its own pinned table upload; the difference of the two calls is the overlay launch"}))


def _child(argv, limit, root=None):
    """One GPU-using step: a fresh process of this file under its own time limit, on this tree's package or on the one under
    `root`. Returns its result dict, or raises."""
    env = dict(os.environ, HAFF_AB_ROOT=os.path.abspath(root)) if root else None
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, capture_output=True, text=True, timeout=limit,
                       cwd=os.path.abspath(root) if root else HERE, env=env)
    if p.returncode != 0:
        raise RuntimeError(f"{argv}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("__RESULT__")][-1]
    return json.loads(line[len("__RESULT__"):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit: its --score_only alternates with this tree's")
    ap.add_argument("--parent_reps", type=int, default=6)
    ap.add_argument("--routes", nargs="+", default=["score_only", "visualize", "files"], choices=["score_only", "visualize", "files"])
    ap.add_argument("--frames", type=int, default=100)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--kernel_reps", type=int, default=30)
    ap.add_argument("--limit", type=int, default=240, help="time limit of each child process, seconds")
    ap.add_argument("--out", default=os.path.join(HERE, "profiles", "visualize_ab.json"))
    ap.add_argument("--worker", default=None)
    ap.add_argument("--bench", default=None)
    ap.add_argument("--work", default=None)
    ap.add_argument("--frame_hw", type=int, nargs=2, default=(256, 256))
    ap.add_argument("--kernel_frames", type=int, default=8)
    a = ap.parse_args()
    if a.worker in ("score_only", "visualize", "files"):
        return worker_route(a.worker, a.bench, a.work, a.batch)
    if a.worker == "kernel":
        return worker_kernel(tuple(a.frame_hw), a.kernel_frames, a.kernel_reps)
    with tempfile.TemporaryDirectory() as tmp:
        bench = os.path.join(tmp, "bench")
        score_ab.make_tree(bench, a.frames)
        runs = []
        for rep in range(a.reps):
            for route in a.routes:
                work = os.path.join(tmp, f"{route}{rep}")
                os.makedirs(work)
                runs.append(_child(["--worker", route, "--bench", bench, "--work", work, "--batch", str(a.batch)], a.limit))
                print(json.dumps(runs[-1]), flush=True)
        versus = []
        for rep in range(a.parent_reps if a.parent else 0):
            for who, root in (("this", None), ("parent", a.parent)):
                work = os.path.join(tmp, f"{who}{rep}")
                os.makedirs(work)
                versus.append(_child(["--worker", "score_only", "--bench", bench, "--work", work, "--batch", str(a.batch)], a.limit, root))
                versus[-1]["tree"] = who
                print(json.dumps(versus[-1]), flush=True)
        kernels = []
        for hw, n in (((256, 256), a.kernel_frames), ((1080, 1920), a.kernel_frames)):
            kernels.append(_child(["--worker", "kernel", "--frame_hw", str(hw[0]), str(hw[1]), "--kernel_frames", str(n),
                                            "--kernel_reps", str(a.kernel_reps)], a.limit))
            print(json.dumps(kernels[-1]), flush=True)
    fps = {r: [a.frames / x["route_s"] for x in runs if x["route"] == r] for r in a.routes}
    out = {"what": "overlay panels end to end and on the device, one MI355X, tiny synthetic model, forced [SEG]; see tools/visualize_ab.py",
           "frames": a.frames, "batch": a.batch, "reps": a.reps, "frames_per_s": fps, "runs": runs, "overlay_launch": kernels,
           "not_measured": ["a 7B / 13B model (the model's own time is the same in every route)", "real ActAffordance frames",
                            "more than one GPU"] + ([] if a.parent else ["the parent commit's --score_only (--parent)"])}
    if versus:
        out["score_only_vs_parent"] = {
            "what": "--score_only of this tree and of the parent commit alternating, each run a fresh process, behind the routes above",
            "frames_per_s": {w: [a.frames / x["route_s"] for x in versus if x["tree"] == w] for w in ("this", "parent")}, "runs": versus}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"frames_per_s": fps, "overlay_launch_s": [k["overlay_launch_s"] for k in kernels]}))


if __name__ == "__main__":
    main()
