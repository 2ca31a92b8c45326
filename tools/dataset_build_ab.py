#!/usr/bin/env python3
"""What `dataset_build build` costs on its two routes, on one MI355X:

  host    : --route host    cvlite: pad, nearest resize, AND, dilation and the Suzuki-Abe contour walk in numpy / Python
  device  : --route device  haff_affordance_extract for the mask arithmetic, ContourReader for the four contour lists

on generated trees (the layout of dataset_build's docstring) of bimanual sequences at 256 x 456 and at 855 x 855, masks that are
unions of discs, hand masks of another size (so the pad and the nearest resize run), k = 5. Both routes run in ONE process after a
warm-up of each, alternating, and every run includes its file time: PNG decoding, the kernels or cvlite, the contour walk, the JSON
and the record file. The split is dataset_build's own clock (every phase ends in a device synchronise). The outputs of the two
routes are compared byte for byte (the JSON) before any number is reported.

And the kernel alone: haff_affordance_extract on 16 planes of 855 x 855 and of 1024 x 1024 with a hand of the same shape and an
output, k = 5, timed with device events after a warm-up, against its traffic floor of 3 B per pixel (read `in`, gather `hand`,
write `out`) at the measured HBM copy rate.

  python tools/dataset_build_ab.py --out profiles/dataset_build_ab.json
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

HBM_COPY_BYTES_PER_S = 6.29e12    # float4 copy, measured (tools/smooth_ab.py); the spec peak is 8.0e12
K = 5
VERBS = "id,key,instances\n0,take,\"['take', 'pick-up']\"\n"


def discs(np, rng, hw, n, r_lo, r_hi, centre=None, spread=0.25):
    H, W = hw
    yy, xx = np.mgrid[0:H, 0:W]
    out = np.zeros(hw, bool)
    cy, cx = centre if centre is not None else (H / 2, W / 2)
    for _ in range(n):
        y, x = cy + rng.normal() * spread * H, cx + rng.normal() * spread * W
        r = rng.uniform(r_lo, r_hi) * min(H, W)
        out |= (yy - y) ** 2 + (xx - x) ** 2 <= r * r
    return out.astype(np.uint8) * 255


def make_tree(root, hw, n, seed=0):
    import numpy as np
    from PIL import Image
    rng = np.random.default_rng(seed)
    H, W = hw
    paths = {k: os.path.join(root, k) for k in ("C", "H", "O", "S")}
    for k in ("C", "H", "O"):
        for side in ("left", "right"):
            os.makedirs(os.path.join(paths[k], side))
    hand_hw = (H * 3 // 4, W * 3 // 4 + 5)
    for i in range(n):
        name = f"{i:07d}"
        for j, side in enumerate(("left", "right")):
            centre = (H / 2, W * (0.3 + 0.4 * j))
            obj = discs(np, rng, hw, 4, 0.08, 0.2, centre, 0.08)
            Image.fromarray(obj).save(os.path.join(paths["O"], side, name + ".png"))
            Image.fromarray(obj).save(os.path.join(paths["C"], side, name + ".png"))
            S = max(hand_hw)                                  # where the object's centre lands in the hand mask: pad, then resize
            hc = (centre[0] * S / H - (S - hand_hw[0] if hand_hw[0] <= hand_hw[1] else 0),
                  centre[1] * S / W - (S - hand_hw[1] if hand_hw[0] > hand_hw[1] else 0))
            Image.fromarray(discs(np, rng, hand_hw, 3, 0.08, 0.15, hc, 0.04)).save(os.path.join(paths["H"], side, name + ".png"))
        seq = os.path.join(paths["S"], name)
        os.makedirs(seq)
        with open(os.path.join(seq, "annotation.json"), "w") as fh:
            json.dump({"taxonomy": [0, 0, 1, 0], "noun": "cup", "verb": "take", "narration": "take the cup", "obj_left": "cup",
                       "obj_right": "pan", "vector": None}, fh)
        Image.fromarray(rng.integers(0, 256, (H, W, 3)).astype(np.uint8)).save(os.path.join(seq, "inpainted_frame.png"))
    paths["csv"] = os.path.join(root, "verbs.csv")
    with open(paths["csv"], "w") as fh:
        fh.write(VERBS)
    return paths


def worker_routes(sizes, reps):
    import torch
    import haff  # noqa: F401
    from haff import dataset_build as D
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for (H, W, n) in sizes:
            p = make_tree(os.path.join(tmp, f"tree{H}x{W}"), (H, W), n)
            warm = make_tree(os.path.join(tmp, f"warm{H}x{W}"), (H, W), 2, seed=1)

            def run(route_name, paths, tag):
                route = D.make_route(route_name)
                out = os.path.join(tmp, f"out_{H}x{W}_{tag}")
                t0 = time.perf_counter()
                res = D.build(paths["C"], paths["H"], paths["O"], paths["S"], K, out, "set", 1e9, ["all"], paths["csv"], route,
                              batch=16, log=lambda *a: None)
                torch.cuda.synchronize()
                total = time.perf_counter() - t0
                with open(os.path.join(out, "jsons", "set.json"), "rb") as fh:
                    blob = fh.read()
                return {"route": route_name, "total_s": total, "phases_s": dict(route.seconds), "valid": res["valid"],
                        "host_extracts": route.host_extracts, "host_walks": route.host_walks}, blob
            for name in ("host", "device"):
                run(name, warm, f"warm_{name}")
            runs, blobs = [], {}
            for rep in range(reps):
                for name in ("host", "device"):
                    r, blob = run(name, p, f"{name}{rep}")
                    if blobs.setdefault("first", blob) != blob:
                        raise RuntimeError(f"{name} route wrote another JSON at {H}x{W}")
                    r["samples_per_s"] = n / r["total_s"]
                    runs.append(r)
                    print(json.dumps(r), flush=True)
            rows.append({"H": H, "W": W, "sequences": n, "k": K, "runs": runs,
                         "samples_per_s": {name: [r["samples_per_s"] for r in runs if r["route"] == name] for name in ("host", "device")}})
    print("__RESULT__" + json.dumps(rows))


def worker_kernel(iters):
    import numpy as np
    import torch
    import haff  # noqa: F401
    from haff import ops
    dev = torch.device("cuda", 0)
    rows = []
    for side in (855, 1024):
        rng = np.random.default_rng(side)
        planes = [torch.from_numpy(discs(np, rng, (side, side), 4, 0.08, 0.2)).to(dev) for _ in range(16)]
        hands = [torch.from_numpy(discs(np, rng, (side, side), 3, 0.1, 0.25)).to(dev) for _ in range(16)]
        tables = ops.nearest_pad_tables((side, side), (side, side), device=dev)
        outs = [torch.empty_like(p) for p in planes]
        items = [(p, h, tables, o) for p, h, o in zip(planes, hands, outs)]
        stats = torch.empty((16, 8), dtype=torch.int64, device=dev)
        for _ in range(5):
            ops.affordance_extract(items, K, stats=stats)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
        ev[0].record()
        for i in range(iters):
            ops.affordance_extract(items, K, stats=stats)     # the descriptor upload and both launches, as dataset_build calls it
            ev[i + 1].record()
        torch.cuda.synchronize()
        ms = sorted(ev[i].elapsed_time(ev[i + 1]) for i in range(iters))
        pixels = 16 * side * side
        floor_ms = 3.0 * pixels / HBM_COPY_BYTES_PER_S * 1e3
        rows.append({"planes": 16, "side": side, "k": K, "iters": iters, "median_ms": ms[iters // 2], "min_ms": ms[0], "max_ms": ms[-1],
                     "traffic_floor_ms": floor_ms, "times_the_floor": ms[iters // 2] / floor_ms,
                     "pixels_per_s": pixels / (ms[iters // 2] * 1e-3)})
    print("__RESULT__" + json.dumps({"kernel": "haff_affordance_extract, k = 5, a hand of the plane's shape, output written",
                                     "floor": "3 B per pixel at 6.29 TB/s (measured float4 copy)", "rows": rows}))


def _child(argv, limit):
    """One GPU-using step: a fresh process of this file under its own time limit. Returns its result, or raises."""
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, capture_output=True, text=True, timeout=limit, cwd=ROOT)
    if p.returncode != 0:
        raise RuntimeError(f"{argv}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("__RESULT__")][-1]
    return json.loads(line[len("__RESULT__"):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", type=int, default=48, help="sequences at 256 x 456")
    ap.add_argument("--large", type=int, default=16, help="sequences at 855 x 855")
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--kernel_iters", type=int, default=200)
    ap.add_argument("--limit", type=int, default=420, help="time limit of each child process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dataset_build_ab.json"))
    ap.add_argument("--worker", default=None)
    a = ap.parse_args()
    if a.worker == "routes":
        return worker_routes([(256, 456, a.small), (855, 855, a.large)], a.reps)
    if a.worker == "kernel":
        return worker_kernel(a.kernel_iters)
    kernel = _child(["--worker", "kernel", "--kernel_iters", str(a.kernel_iters)], a.limit)
    print(json.dumps(kernel), flush=True)
    routes = _child(["--worker", "routes", "--small", str(a.small), "--large", str(a.large), "--reps", str(a.reps)], a.limit)
    out = {"what": "dataset_build build on its host and device routes, file time included, and haff_affordance_extract alone; one "
                   "MI355X; see tools/dataset_build_ab.py",
           "routes": routes, "kernel_alone": kernel,
           "not_measured": ["real 2HANDS masks and frames", "JPEG or video decoding", "more than one GPU", "k other than 5"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"samples_per_s": {f"{r['H']}x{r['W']}": r["samples_per_s"] for r in routes}, "kernel_alone": kernel["rows"]}))


if __name__ == "__main__":
    main()
