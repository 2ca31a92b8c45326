#!/usr/bin/env python3
"""A/B of the two routes from a mask plane on the device to its 2HANDS contours, on one MI355X, alternating in one process:

  host   : the plane read back, cvlite.find_contours_external in Python (the only route before haff_contour_extract)
  device : haff.contours.ContourReader (ops.contour_extract; two small tables and the used vertex prefixes read back)

The planes are the golden sample's eleven aff_* / obj_* planes and the 855 x 855 disc unions tools/score_ab.py generates. Both routes
must return the same lists; the tool stops if they do not. There is no pass mark: the numbers are written down.

  python tools/contours_ab.py --discs 6 --reps 2 --out profiles/contours_ab.json
  rocprofv3 --kernel-trace --stats -d <dir> -o run --output-format csv -- python tools/contours_ab.py --worker device
  python tools/contours_ab.py ... --kernel-stats <dir>/.../run_kernel_stats.csv     # folds the stage times into the JSON
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SAMPLE = os.path.join(ROOT, "tests", "golden", "actaffordance_sample")
STAGES = ("ch_setup_kernel", "label_tile_kernel", "label_seam_kernel", "label_root_kernel", "extract_start_kernel",
          "extract_number_kernel", "extract_walk_kernel", "extract_offsets_kernel")


def planes(n_discs, seed=0):
    """[(name, uint8 plane)]: the sample's mask planes, then score_ab.make_tree's disc unions."""
    import numpy as np
    from PIL import Image
    out = []
    for path in sorted(glob.glob(os.path.join(SAMPLE, "*", "*", "*.png"))):
        if os.path.basename(path).startswith(("aff_", "obj_")):
            out.append((os.path.relpath(path, SAMPLE), (np.array(Image.open(path).convert("L")) > 0).astype(np.uint8) * 255))
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:855, :855]
    for i in range(n_discs):
        m = np.zeros((855, 855), bool)
        for _ in range(3):
            cy, cx, r = rng.uniform(0, 855, 2).tolist() + [rng.uniform(60, 250)]
            m |= (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
        out.append((f"discs{i}", m.astype(np.uint8) * 255))
    return out


def kernel_stats(path):
    """{stage: {"calls", "total_us", "mean_us"}} from a rocprofv3 kernel_stats.csv, the extraction's kernels only."""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            for stage in STAGES:
                if stage in name:
                    key = stage + (("<store>" if "<true>" in name else "<count>") if stage == "extract_walk_kernel" else "")
                    out[key] = {"calls": int(row["Calls"]), "total_us": float(row["TotalDurationNs"]) / 1e3,
                                "mean_us": float(row["AverageNs"]) / 1e3}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--discs", type=int, default=6)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "contours_ab.json"))
    ap.add_argument("--worker", default=None, choices=["device"], help="the device route alone, three times: the run to trace")
    ap.add_argument("--kernel-stats", default=None, help="a rocprofv3 kernel_stats.csv of a --worker device run")
    a = ap.parse_args()
    import numpy as np
    import torch
    import haff  # noqa: F401
    from haff import contours, cvlite
    named = planes(a.discs)
    dev = [torch.from_numpy(m).cuda() for _, m in named]
    reader = contours.ContourReader()
    reader.read(dev)                                            # warm-up: library load, workspace
    torch.cuda.synchronize()
    if a.worker:
        for _ in range(3):
            reader.read(dev)
        torch.cuda.synchronize()
        return print(json.dumps({"planes": len(dev), "host_walks": reader.host_walks}))
    runs = {"host": [], "device": []}
    for _ in range(a.reps):
        t0 = time.perf_counter()
        host = [cvlite.find_contours_external(p.cpu().numpy()) for p in dev]
        runs["host"].append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        got = reader.read(dev)
        runs["device"].append(time.perf_counter() - t0)
        for (name, _), g, h in zip(named, got, host):
            if len(g) != len(h) or not all(np.array_equal(x, y) for x, y in zip(g, h)):
                raise SystemExit(f"{name}: the two routes differ")
    out = {"what": "mask plane on the device -> external contours, host route against ContourReader, one MI355X; see tools/contours_ab.py",
           "planes": len(dev), "shapes": sorted({"%dx%d" % m.shape for _, m in named}),
           "contours": [len(c) for c in host], "vertices": [int(sum(len(x) for x in c)) for c in host], "reps": a.reps,
           "seconds": runs, "planes_per_s": {k: [len(dev) / s for s in v] for k, v in runs.items()},
           "host_walks": reader.host_walks, "routes_equal": True,
           "kernel_stats": kernel_stats(a.kernel_stats) if a.kernel_stats else None,
           "not_measured": ["predicted masks of a trained model", "more than one GPU"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"planes_per_s": out["planes_per_s"], "host_walks": out["host_walks"], "kernel_stats": out["kernel_stats"]}))


if __name__ == "__main__":
    main()
