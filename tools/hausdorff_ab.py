#!/usr/bin/env python3
"""A/B of the three scoring routes of inference.py on one MI355X, end to end, on the tree tools/score_ab.py generates (256 x 256
frames, 855 x 855 disc-union masks; the tiny synthetic model with a forced [SEG] answer):

  plain  : --score_only                            IoU / IoCM only
  host   : --score_only --score_hausdorff          the union planes read back per batch, evaluation.calculate_hausdorff in a thread
  device : --score_only --score_hausdorff_device   contour walk and point-set distance in HIP, one read-back at the end

The routes alternate, each run a fresh child process under its own time limit; a run that fails or times out ends the job. The
host route walks six 855 x 855 planes per frame in Python, so the frame count is small. `--worker device` without --bench runs
the device route once on a tree of its own: the run to put under a kernel trace (profiles/hausdorff_kernel_stats.json).

  python tools/hausdorff_ab.py --frames 48 --reps 2 --out profiles/hausdorff_ab.json
  rocprofv3 --kernel-trace --stats -d <dir> -o run --output-format csv -- python tools/hausdorff_ab.py --worker device --frames 48
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

ROUTES = {"plain": [], "host": ["--score_hausdorff"], "device": ["--score_hausdorff_device"]}


def worker(route, bench, batch):
    import contextlib
    import io
    import score_ab
    import haff  # noqa: F401
    from haff import inference, scoring
    score_ab._force_seg()
    clock = score_ab._Clock()
    clock.wrap(inference, "build_model_and_tokenizer", "model_build_s")
    clock.wrap(scoring.BenchmarkScorer, "add_batch", "scorer_add_batch_s")
    clock.wrap(scoring.BenchmarkScorer, "report", "scorer_report_s")
    made = []
    init = scoring.BenchmarkScorer.__init__

    def recorded(self, *a, **kw):
        init(self, *a, **kw)
        made.append(self)
    scoring.BenchmarkScorer.__init__ = recorded
    argv = ["--synthetic", "tiny", "--benchmark-dir", bench, "--vis_save_path", os.path.join(bench, "..", "th"), "--image_size", "224",
            "--batch-size", str(batch), "--score_only"] + ROUTES[route]
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(io.StringIO()):
        res = inference.main(argv)
    total = time.perf_counter() - t0
    b = res["best"]
    print("__RESULT__" + json.dumps({"route": route, "total_s": total, "route_s": total - clock.t["model_build_s"], "stages": clock.t,
                                     "count": b["count"], "host_walks": made[0].host_walks,
                                     "best": {k: b[k] for k in ("threshold", "iou", "iocm", "hd", "directed_hd")}}))


def _child(argv, limit):
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, capture_output=True, text=True, timeout=limit, cwd=ROOT)
    if p.returncode != 0:
        raise RuntimeError(f"{argv}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("__RESULT__")][-1]
    return json.loads(line[len("__RESULT__"):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--limit", type=int, default=300, help="time limit of each child process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hausdorff_ab.json"))
    ap.add_argument("--worker", default=None, choices=list(ROUTES))
    ap.add_argument("--bench", default=None)
    a = ap.parse_args()
    if a.worker:
        if a.bench is None:                                   # a stand-alone run of one route (for a kernel trace)
            import score_ab
            with tempfile.TemporaryDirectory() as tmp:
                score_ab.make_tree(os.path.join(tmp, "bench"), a.frames)
                return worker(a.worker, os.path.join(tmp, "bench"), a.batch)
        return worker(a.worker, a.bench, a.batch)
    import score_ab
    with tempfile.TemporaryDirectory() as tmp:
        bench = os.path.join(tmp, "bench")
        score_ab.make_tree(bench, a.frames)
        runs = []
        for rep in range(a.reps):
            for route in ROUTES:
                runs.append(_child(["--worker", route, "--bench", bench, "--batch", str(a.batch)], a.limit))
                print(json.dumps(runs[-1]), flush=True)
    fps = {r: [a.frames / x["route_s"] for x in runs if x["route"] == r] for r in ROUTES}
    same = all(x["best"] == y["best"] for x in runs for y in runs if x["route"] != "plain" and y["route"] != "plain")
    out = {"what": "end-to-end scoring route A/B on one MI355X, tiny synthetic model, forced [SEG]; see tools/hausdorff_ab.py",
           "frames": a.frames, "batch": a.batch, "reps": a.reps, "frames_per_s": fps,
           "host_and_device_reports_equal": same, "runs": runs,
           "not_measured": ["real ActAffordance frames", "more than one GPU", "a 7B / 13B model (the model's own time is the same in "
                            "every route)"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"frames_per_s": fps, "host_and_device_reports_equal": same}))


if __name__ == "__main__":
    main()
