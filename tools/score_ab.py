#!/usr/bin/env python3
"""A/B of the two routes from a checkpoint to the benchmark's numbers, end to end, on one MI355X:

  files  : inference.py (PNG planes per threshold) then evaluation.py --map over the written tree   (the route before --score)
  device : inference.py --score_only (haff_score_masks per batch, one host read at the end)

on a generated ActAffordance-shaped tree (256 x 256 frames, 855 x 855 disc-union masks), the tiny synthetic model with a forced
[SEG] answer (the model's own time is the same in both routes and small here: what differs is everything after it). The routes
alternate, each run a fresh child process under its own time limit; a run that fails or times out ends the job. The Hausdorff
distances are left out of both routes (evaluation.calculate_hausdorff stubbed in the files route: the Python contour walk would
dominate it; --score_only does not compute them either). Validation is timed the same way: train_ds.validate at --val_batch_size
1 and 8 against the former per-sample host loop, restated here.

  python tools/score_ab.py --frames 200 --reps 2 --out profiles/score_ab.json
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


def make_tree(root, n_frames, seed=0):
    import numpy as np
    from PIL import Image
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[:855, :855]
    for i in range(n_frames):
        leaf = os.path.join(root, f"video{i // 25:02d}", f"{i:07d}")
        os.makedirs(leaf)
        Image.fromarray(rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)).save(os.path.join(leaf, "inpainting.png"))
        with open(os.path.join(leaf, "annotation.json"), "w") as f:
            json.dump({"narration": f"pick up object {i % 17}"}, f)
        for side in ("left", "right"):
            m = np.zeros((855, 855), bool)
            for _ in range(3):
                cy, cx, r = rng.uniform(0, 855, 2).tolist() + [rng.uniform(60, 250)]
                m |= (yy - cy) ** 2 + (xx - cx) ** 2 < r * r
            Image.fromarray(m.astype(np.uint8) * 255).save(os.path.join(leaf, f"aff_{side}.png"))


class _Clock:
    """Wall time spent inside wrapped functions (host stages of a route)."""

    def __init__(self):
        self.t = {}

    def wrap(self, owner, name, key):
        fn = getattr(owner, name)

        def timed(*a, **kw):
            t0 = time.perf_counter()
            try:
                return fn(*a, **kw)
            finally:
                self.t[key] = self.t.get(key, 0.0) + time.perf_counter() - t0
        setattr(owner, name, timed)


def _force_seg():
    import torch
    from haff import lisa
    orig = lisa.LisaMI355.evaluate

    def evaluate(self, *a, **kw):
        kw["forced_answer"] = torch.tensor([[5, self.cfg.seg_token_idx, self.cfg.eos_token_id]]).expand(a[2].shape[0], -1)
        kw["max_new_tokens"] = 3
        return orig(self, *a, **kw)
    lisa.LisaMI355.evaluate = evaluate


def worker_route(route, bench, work, batch):
    import contextlib
    import io
    import torch
    import haff  # noqa: F401
    from haff import evaluation, inference, scoring
    _force_seg()
    clock = _Clock()
    clock.wrap(inference, "build_model_and_tokenizer", "model_build_s")
    clock.wrap(inference, "load_rgb", "frame_decode_s")
    argv = ["--synthetic", "tiny", "--benchmark-dir", bench, "--vis_save_path", os.path.join(work, "th"), "--image_size", "224",
            "--batch-size", str(batch)]
    sink = io.StringIO()
    t0 = time.perf_counter()
    if route == "files":
        clock.wrap(inference, "output_planes", "planes_readback_s")
        clock.wrap(inference, "save_mask", "png_encode_s")
        evaluation.calculate_hausdorff = lambda a, b: (0.0, 0.0)
        with contextlib.redirect_stdout(sink):
            inference.main(argv)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            res = evaluation.main(["--benchmark_folder", bench, "--comparison_folder", work, "--map"])
        clock.t["evaluation_s"] = time.perf_counter() - t1
    else:
        clock.wrap(scoring.BenchmarkScorer, "add_batch", "scorer_add_batch_s")
        clock.wrap(scoring.BenchmarkScorer, "report", "scorer_report_s")
        with contextlib.redirect_stdout(sink):
            res = inference.main(argv + ["--score_only"])
    total = time.perf_counter() - t0
    out = {"route": route, "total_s": total, "route_s": total - clock.t["model_build_s"], "stages": clock.t,
           "count": res["best"]["count"], "mean_average_precision": res["mean_average_precision"],
           "best": {k: res["best"][k] for k in ("threshold", "iou", "iocm")}}
    print("__RESULT__" + json.dumps(out))


def _validate_host(model, dataset, tokenizer, args, device):
    """The per-sample host loop validate() ran before the device scorer (four planes to the host per sample)."""
    import numpy as np
    import torch
    from haff import train_ds
    model.eval()
    iou_m, iocm_m = train_ds.AverageMeter("IoU"), train_ds.AverageMeter("IoCM")
    with torch.no_grad():
        for idx in range(len(dataset)):
            batch = train_ds.collate_fn([dataset[idx]], tokenizer, args.model_max_length, conv_type=args.conv_type)
            batch = {k: (v.to(device) if torch.is_tensor(v) else v) for k, v in batch.items()}
            out = model(**batch)
            t = int(out["pred_taxonomies"][0][0].argmax())
            left = (out["pred_masks_left"][0][0] > 0).cpu().numpy()
            right = (out["pred_masks_right"][0][0] > 0).cpu().numpy()
            if t == 1:
                left[:] = False
            if t == 0:
                right[:] = False
            pred = np.logical_or(left, right)
            gt = np.logical_or(out["gt_masks_left"][0][0].cpu().numpy() > 0, out["gt_masks_right"][0][0].cpu().numpy() > 0)
            iou_m.update(train_ds.calculate_iou(pred, gt))
            iocm_m.update(train_ds.calculate_iocm(gt, pred))
    model.train()
    return iou_m.avg, iocm_m.avg


def worker_validate(n_samples, mask_hw, reps):
    import torch
    import haff  # noqa: F401
    from haff import checkpoint, config as hcfg, train_ds
    from haff.train_model import LisaTrainable
    device = torch.device("cuda", 0)
    torch.cuda.set_device(0)
    cfg = hcfg.tiny()
    tokenizer = checkpoint.ByteTokenizer(cfg)
    sd = checkpoint.synthetic_state_dict(cfg, 1234, device, torch.bfloat16)
    model = LisaTrainable(cfg, sd, dtype=torch.bfloat16, device=device, lora_r=8, lora_alpha=16, lora_dropout=0.05, seed=0)
    ds = train_ds.SyntheticAffDataset(cfg, n_samples, 777, mask_hw, inference=True)
    runs = {"host_loop": [], "device_vbs1": [], "device_vbs8": []}
    values = {}
    for rep in range(reps + 1):               # the first round warms every path up and is not reported
        for key, vbs in (("host_loop", None), ("device_vbs1", 1), ("device_vbs8", 8)):
            args = train_ds.parse_args(["--synthetic", "tiny", "--val_batch_size", str(vbs or 1)])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if vbs is None:
                v = _validate_host(model, ds, tokenizer, args, device)
            else:
                v = train_ds.validate(model, ds, tokenizer, args, 0, 1, device)
            torch.cuda.synchronize()
            if rep:
                runs[key].append(time.perf_counter() - t0)
            values[key] = [float(v[0]), float(v[1])]
    print("__RESULT__" + json.dumps({"samples": n_samples, "mask_hw": list(mask_hw), "seconds": runs, "iou_iocm": values}))


def _child(argv, limit):
    """One GPU-using step: a fresh process under its own time limit. Returns its result dict, or raises."""
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + argv, capture_output=True, text=True, timeout=limit, cwd=ROOT)
    if p.returncode != 0:
        raise RuntimeError(f"{argv}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-4000:]}")
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("__RESULT__")][-1]
    return json.loads(line[len("__RESULT__"):])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=200)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--val_samples", type=int, default=32)
    ap.add_argument("--val_mask_hw", type=int, nargs=2, default=(480, 640))
    ap.add_argument("--limit", type=int, default=240, help="time limit of each child process, seconds")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_ab.json"))
    ap.add_argument("--worker", default=None)
    ap.add_argument("--bench", default=None)
    ap.add_argument("--work", default=None)
    a = ap.parse_args()
    if a.worker in ("files", "device"):
        return worker_route(a.worker, a.bench, a.work, a.batch)
    if a.worker == "validate":
        return worker_validate(a.val_samples, tuple(a.val_mask_hw), a.reps)
    with tempfile.TemporaryDirectory() as tmp:
        bench = os.path.join(tmp, "bench")
        t0 = time.perf_counter()
        make_tree(bench, a.frames)
        runs = []
        for rep in range(a.reps):
            for route in ("files", "device"):
                work = os.path.join(tmp, f"{route}{rep}")
                os.makedirs(work)
                runs.append(_child(["--worker", route, "--bench", bench, "--work", work, "--batch", str(a.batch)], a.limit))
                print(json.dumps(runs[-1]), flush=True)
        val = _child(["--worker", "validate", "--val_samples", str(a.val_samples), "--val_mask_hw", *map(str, a.val_mask_hw),
                      "--reps", str(a.reps)], a.limit)
        print(json.dumps(val), flush=True)
    fps = {r: [a.frames / x["route_s"] for x in runs if x["route"] == r] for r in ("files", "device")}
    out = {"what": "end-to-end route A/B on one MI355X, tiny synthetic model, forced [SEG]; see tools/score_ab.py",
           "frames": a.frames, "batch": a.batch, "reps": a.reps, "tree_build_s": time.perf_counter() - t0,
           "frames_per_s": fps, "runs": runs, "validation": val,
           "not_measured": ["Hausdorff distances (left out of both routes)", "a 7B / 13B model (the model's own time is the same in "
                            "both routes)", "real ActAffordance frames", "more than one GPU"]}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps({"frames_per_s": fps, "validation_s": val["seconds"]}))


if __name__ == "__main__":
    main()
