#!/usr/bin/env python3
"""What --device_png costs and what it replaces, on one MI355X (in the style of tools/smooth_ab.py, whose helpers it uses):

  plain  : inference.py                  (the yardstick: ten planes per frame read back, Pillow encodes each on the main thread)
  device : inference.py --device_png     (haff_png_measure + haff_png_emit once per chunk, the PNG streams read back, png.wrap)

on two generated trees, one of 256 x 256 frames and one of 1080 x 1920 frames (the masks are written at the frame's size, so the
small tree alone would measure overheads), a synthetic model (--model, default 7b) with a forced [SEG] answer, four frames per
evaluate(). The routes alternate, each run a fresh child process under its own time limit; a run that fails or times out ends the
job. The parent then opens every file of the first pair of runs and compares pixels, and reports the file sizes of both routes.

And the two calls alone: ten disc-union planes of 855 x 855 and of 1080 x 1920, each call timed with device events after a warm-up,
against its read floor of 1 B per pixel at the measured HBM copy rate.

  python tools/device_png_ab.py --frames 24 --reps 2 --out profiles/device_png_ab.json
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
import score_ab   # noqa: E402  (_Clock, _force_seg)

HBM_COPY_BYTES_PER_S = 6.29e12    # float4 copy, measured; the spec peak is 8.0e12
ROUTES = ("plain", "device")
TREES = {"256x256": (256, 256), "1080x1920": (1080, 1920)}


def make_tree(root, n_frames, hw, seed=0):
    """An ActAffordance-shaped tree of frames of one size: blocky colour noise (cheap to decode), a narration each."""
    import numpy as np
    from PIL import Image
    rng = np.random.default_rng(seed)
    H, W = hw
    for i in range(n_frames):
        leaf = os.path.join(root, f"video{i // 25:02d}", f"{i:07d}")
        os.makedirs(leaf)
        coarse = rng.integers(0, 256, ((H + 31) // 32, (W + 31) // 32, 3), dtype=np.uint8)
        Image.fromarray(np.kron(coarse, np.ones((32, 32, 1), np.uint8))[:H, :W]).save(os.path.join(leaf, "inpainting.png"))
        with open(os.path.join(leaf, "annotation.json"), "w") as f:
            json.dump({"narration": f"pick up object {i % 17}"}, f)


def disc_planes(n, hw, device, seed=0):
    """n uint8 planes of 0 / 255 on the device: unions of a few discs, as hand and affordance masks are."""
    import numpy as np
    import torch
    rng = np.random.default_rng(seed)
    H, W = hw
    yy, xx = np.mgrid[:H, :W]
    planes = []
    for _ in range(n):
        m = np.zeros((H, W), bool)
        for _ in range(int(rng.integers(1, 5))):
            cy, cx, r = rng.integers(0, H), rng.integers(0, W), rng.integers(min(H, W) // 16, min(H, W) // 4)
            m |= (yy - cy) ** 2 + (xx - cx) ** 2 <= r * r
        planes.append(torch.from_numpy(m.astype(np.uint8) * 255).to(device))
    return planes


def worker_route(route, bench, work, batch, model):
    import contextlib
    import io
    import torch
    import haff  # noqa: F401
    from haff import inference, png
    score_ab._force_seg()
    clock = score_ab._Clock()
    clock.wrap(inference, "build_model_and_tokenizer", "model_build_s")
    clock.wrap(inference, "load_rgb", "frame_decode_s")
    clock.wrap(inference, "output_planes", "planes_s")               # plain: thresholds + the read-back; device: the enqueue
    clock.wrap(inference, "save_mask", "pillow_encode_write_s")
    clock.wrap(png.PngEncoder, "encode", "device_encode_s")           # both calls, both reads, png.wrap
    clock.wrap(inference, "save_png_bytes", "file_write_s")
    argv = ["--synthetic", model, "--benchmark-dir", bench, "--vis_save_path", os.path.join(work, "th"), "--batch-size", str(batch)]
    if model == "tiny":
        argv += ["--image_size", "224"]
    sink = io.StringIO()
    t0 = time.perf_counter()
    with contextlib.redirect_stdout(sink):
        inference.main(argv + (["--device_png"] if route == "device" else []))
        torch.cuda.synchronize()
    total = time.perf_counter() - t0
    sizes = [os.path.getsize(os.path.join(d, f)) for d, _, fs in os.walk(work) for f in fs]
    out = {"route": route, "total_s": total, "route_s": total - clock.t["model_build_s"], "stages": clock.t, "files": len(sizes),
           "file_bytes": {"total": sum(sizes), "min": min(sizes), "max": max(sizes), "mean": sum(sizes) / len(sizes)}}
    print("__RESULT__" + json.dumps(out))


def worker_kernel(iters):
    import numpy as np
    import torch
    import haff  # noqa: F401
    from haff import ops
    dev = torch.device("cuda", 0)
    rows = []
    for hw in ((855, 855), (1080, 1920)):
        planes = disc_planes(10, hw, dev, seed=hw[0])
        for _ in range(5):
            table_dev, job = ops.png_measure(planes)
            table = table_dev.cpu().numpy().view(np.uint32)
            out = ops.png_emit(job, table)
        torch.cuda.synchronize()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3 * iters)]
        for i in range(iters):
            ev[3 * i].record()
            table_dev, job = ops.png_measure(planes)          # allocates its workspace and table, as the encoder's call does
            ev[3 * i + 1].record()
            ops.png_emit(job, table, out=out)                 # the table is the same every time: no read between the calls here
            ev[3 * i + 2].record()
        torch.cuda.synchronize()
        measure = sorted(ev[3 * i].elapsed_time(ev[3 * i + 1]) for i in range(iters))
        emit = sorted(ev[3 * i + 1].elapsed_time(ev[3 * i + 2]) for i in range(iters))
        pixels = 10 * hw[0] * hw[1]
        floor_ms = pixels / HBM_COPY_BYTES_PER_S * 1e3
        row = {"planes": 10, "H": hw[0], "W": hw[1], "iters": iters, "raw_bytes": pixels, "stream_bytes": int(out.numel()),
               "read_floor_ms": floor_ms}
        for name, ms in (("measure", measure), ("emit", emit)):
            row[name] = {"median_ms": ms[iters // 2], "min_ms": ms[0], "max_ms": ms[-1], "times_the_floor": ms[iters // 2] / floor_ms}
        rows.append(row)
    print("__RESULT__" + json.dumps({"kernel": "haff_png_measure (three launches) and haff_png_emit (a memset and one launch), ten "
                                               "disc-union planes of 0 / 255 per call",
                                     "floor": "1 B per pixel read at 6.29 TB/s (measured float4 copy)", "rows": rows}))


def _child(argv, limit):
    """One GPU-using step: a fresh process of this file under its own time limit. Returns its result dict, or raises."""
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, capture_output=True, text=True, timeout=limit, cwd=ROOT)
    if p.returncode != 0:
        raise RuntimeError(f"{argv}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("__RESULT__")][-1]
    return json.loads(line[len("__RESULT__"):])


def same_pixels(plain, device):
    """Every file of the plain tree has a twin in the device tree with equal pixels, mode L: the count of files compared."""
    import numpy as np
    from PIL import Image
    n = 0
    for d, _, fs in os.walk(plain):
        for f in fs:
            a = Image.open(os.path.join(d, f))
            b = Image.open(os.path.join(device, os.path.relpath(os.path.join(d, f), plain)))
            if b.mode != "L" or not np.array_equal(np.asarray(a), np.asarray(b)):
                raise RuntimeError(f"{os.path.join(d, f)}: the device route's file differs")
            n += 1
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--model", default="7b", choices=["tiny", "mid", "7b", "13b"])
    ap.add_argument("--kernel_iters", type=int, default=100)
    ap.add_argument("--limit", type=int, default=300, help="time limit of each child process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "device_png_ab.json"))
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
    trees = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, hw in TREES.items():
            bench = os.path.join(tmp, "bench" + name)
            make_tree(bench, a.frames, hw)
            runs = []
            for rep in range(a.reps):
                for route in ROUTES:
                    work = os.path.join(tmp, f"{name}{route}{rep}")
                    os.makedirs(work)
                    runs.append(_child(["--worker", route, "--bench", bench, "--work", work, "--batch", str(a.batch),
                                        "--model", a.model], a.limit))
                    runs[-1]["tree"] = name
                    print(json.dumps(runs[-1]), flush=True)
            compared = same_pixels(os.path.join(tmp, f"{name}plain0"), os.path.join(tmp, f"{name}device0"))
            trees[name] = {"frame_hw": list(hw), "frames_per_s": {r: [a.frames / x["route_s"] for x in runs if x["route"] == r] for r in ROUTES},
                           "file_bytes": {r: next(x["file_bytes"] for x in runs if x["route"] == r) for r in ROUTES},
                           "files_compared_pixel_equal": compared, "runs": runs}
    out = {"what": "cost of inference.py --device_png against the same command without it, one MI355X, synthetic model, forced [SEG]; "
                   "see tools/device_png_ab.py",
           "model": a.model, "frames": a.frames, "batch": a.batch, "reps": a.reps, "trees": trees, "kernel_alone": kernel,
           "not_measured": ["robot_demo.py --device_png (its request latency)", "real ActAffordance frames and real checkpoints' masks",
                            "--smooth_masks, --score and --write_records beside --device_png", "planes other than 0 / 255 masks",
                            "more than one GPU"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({name: {"frames_per_s": t["frames_per_s"], "file_bytes": t["file_bytes"]} for name, t in trees.items()}))
    print(json.dumps(kernel["rows"]))


if __name__ == "__main__":
    main()
