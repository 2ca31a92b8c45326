"""Benchmark scoring and validation metrics on the device (csrc/mask_score.hip, ops.score_masks).

`inference.py` used to leave the device three times per frame to be scored: a host read of the taxonomy argmax, ten PNG planes,
and `evaluation.py` decoding and resampling them again to count four integers per frame and threshold. Here the fp32 mask logits
`evaluate()` returns are compared, resampled to the benchmark's 855 x 855 (the 0/255 plane's bilinear resample followed by `> 0`,
in exact integers), gated, ANDed and counted by ONE kernel launch per batch of frames; the counts stay in HBM for the whole run
and are read back once.

  pack_frames      the kernel's per-frame descriptor table (haff_score_frame, include/haff_hip.h) from tensors
  BenchmarkScorer  `evaluation.evaluate_folders` for an inference run: the frame rules of `evaluation.score_frame`, the same
                   accumulation order and the same report dict, from the integer counts
  counts_to_iou    `evaluation.calculate_iou` / `calculate_iocm` on the integers

Relation to evaluation.py: it resamples with fp32 `F.interpolate` (its stand-in for cv2.resize), whose source coordinates carry a few
ulp of error; the device rule is the exact rational value of the same formula. The two can differ only at pixels whose coverage is
within a hair of the tie (tests/test_score_ref_cpu.py bounds the band and its population).

With hausdorff="device" the two Hausdorff distances stay on the device too (csrc/contour_hausdorff.hip, ops.contour_hausdorff): the
contour walk of every predicted union plane and of the frame's ground-truth union, and the two directed point-set distances, as
integers that join the same single read-back; report() takes the square roots.
"""
import math
import os
import sys

import numpy as np
import torch

from . import ops
from . import postprocess
from .contours import host_walk

BENCHMARK_HW = (855, 855)                  # calculate_iou.py:139: the uncropped benchmark resolution


def _plane(t, dtype, name):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live in HBM (cuda tensor); the hot path has no CPU fallback")
    assert t.dtype == dtype and t.is_contiguous(), (name, t.dtype, t.is_contiguous())
    return t


def pack_frames(frames):
    """frames: dicts with the keys left, right (fp32 [Hs, Ws] logits or None), taxonomy (fp32, 4 n values, or None: gate open),
    gt_left, gt_right, obj_left, obj_right (uint8 2-D planes or None), out (uint8 [T, Hb, Wb] or None), target_hw, when
    both hands are None, src_hw, and optionally vis (k >= 1: the frame's overlays are drawn through record k - 1 of pack_vis's
    table; 0 or absent: nothing is drawn). Returns the int64 [n, 16] descriptor table of ops.score_masks; the caller keeps the tensors alive
    until the launch is enqueued. Shapes are recorded as the tensors have them: the library refuses a ground-truth or object plane
    whose shape is not the target's, and sizes it does not take."""
    table = np.zeros((len(frames), ops.SCORE_FRAME_WORDS), dtype=np.int64)
    ints = table.view(np.int32).reshape(len(frames), 2 * ops.SCORE_FRAME_WORDS)
    for i, f in enumerate(frames):
        left, right = _plane(f.get("left"), torch.float32, "left"), _plane(f.get("right"), torch.float32, "right")
        src = left if left is not None else right
        hs, ws = (src.shape if src is not None else f.get("src_hw", (1, 1)))
        assert src is None or src.dim() == 2
        assert left is None or right is None or left.shape == right.shape
        tax = _plane(f.get("taxonomy"), torch.float32, "taxonomy")
        out = _plane(f.get("out"), torch.uint8, "out")
        hb, wb = f["target_hw"]
        assert out is None or (out.dim() == 3 and tuple(out.shape[1:]) == (hb, wb))
        ptrs = [left, right, tax]
        shapes = []
        for key in ("gt_left", "gt_right", "obj_left", "obj_right"):
            p = _plane(f.get(key), torch.uint8, key)
            assert p is None or p.dim() == 2
            ptrs.append(p)
            shapes += list(p.shape) if p is not None else [0, 0]
        ptrs.append(out)
        table[i, :8] = [0 if p is None else p.data_ptr() for p in ptrs]
        ints[i, 16:29] = [hs, ws, hb, wb, 0 if tax is None else tax.numel()] + shapes
        ints[i, 29] = int(f.get("vis") or 0)
    return table


OVERLAY_ALPHA, OVERLAY_BETA, OVERLAY_GAMMA = (0.5, 1.0), (0.5, 0.5), 0.0   # calculate_iou.py:81-82: the two cv2.addWeighted calls
OVERLAY_COLORS = ((255, 0, 0), (0, 255, 0))   # RGB, left and right: green as the code at :77-78 does, not blue as its comment says


def pack_vis(records):
    """The overlay records of ops.score_masks (haff_score_vis, include/haff_hip.h) as an int64 [m, 16] table. records: dicts with
    rgb (uint8 [Hf, Wf, 3], the frame as loaded), row / col (int32 [Hf] / [Wf] nearest indices into the frame's target grid, as
    cvlite.nearest_indices gives them; both None for the identity), out = (benchmark overlay, prediction overlay), each a uint8
    view [Hf, Wf, 3] whose pixels are contiguous and whose rows may be strided (the two halves of one [Hf, 2 Wf, 3] canvas, say) or
    None (not drawn), t (index of the threshold that is drawn) and optionally alpha, beta, gamma, colors (create_overlay's by
    default). Everything lives in HBM and is kept alive by the caller until the launch is enqueued."""
    table = np.zeros((len(records), ops.SCORE_FRAME_WORDS), dtype=np.int64)
    ints = table.view(np.int32).reshape(len(records), 2 * ops.SCORE_FRAME_WORDS)
    floats = table.view(np.float32).reshape(len(records), 2 * ops.SCORE_FRAME_WORDS)
    for i, r in enumerate(records):
        rgb = _plane(r["rgb"], torch.uint8, "rgb")
        assert rgb.dim() == 3 and rgb.shape[2] == 3
        hf, wf = rgb.shape[:2]
        row, col = _plane(r.get("row"), torch.int32, "row"), _plane(r.get("col"), torch.int32, "col")
        assert row is None or tuple(row.shape) == (hf,)
        assert col is None or tuple(col.shape) == (wf,)
        table[i, :3] = [rgb.data_ptr(), 0 if row is None else row.data_ptr(), 0 if col is None else col.data_ptr()]
        for k, o in enumerate(r["out"]):
            if o is None:
                continue
            if not o.is_cuda:
                raise RuntimeError("out must live in HBM (cuda tensor); the hot path has no CPU fallback")
            assert o.dtype == torch.uint8 and tuple(o.shape) == (hf, wf, 3) and o.stride(2) == 1 and o.stride(1) == 3
            table[i, 3 + k], table[i, 5 + k] = o.data_ptr(), o.stride(0) if hf > 1 else max(o.stride(0), 3 * wf)
        ints[i, 14:17] = [hf, wf, int(r["t"])]
        floats[i, 17:22] = [*r.get("alpha", OVERLAY_ALPHA), *r.get("beta", OVERLAY_BETA), r.get("gamma", OVERLAY_GAMMA)]
        ints[i, 22:28] = np.asarray(r.get("colors", OVERLAY_COLORS), dtype=np.int32).reshape(6)
    return table


def counts_to_iou(inter, union, area):
    """evaluation.calculate_iou / calculate_iocm from the counts: float(inter) / float(denominator), 0.0 on an empty one."""
    inter, union, area = int(inter), int(union), int(area)
    return (float(inter) / float(union) if union != 0 else 0.0), (float(inter) / float(area) if area != 0 else 0.0)


def report_from_frames(names, frames, want_hausdorff):
    """evaluation.evaluate_folders' result from per-frame results. names: the threshold folder names; frames: per scored frame, in
    the benchmark's sorted folder order, (label, counts int [T, 4], hausdorff [T] of (directed, symmetric) or None). The thresholds
    are reported in sorted name order, as evaluate_folders lists the comparison folder."""
    order = sorted(range(len(names)), key=lambda k: names[k])
    per_th = []
    for k in order:
        tot = np.zeros(4)
        count = zero = 0
        for _, counts, hd in frames:
            iou, iocm = counts_to_iou(counts[k][0], counts[k][1], counts[k][2])
            dhd, shd = hd[k] if want_hausdorff else (0.0, 0.0)
            tot += np.asarray((iou, iocm, dhd, shd))
            zero += int(iou == 0 and iocm == 0)
            count += 1
        avg = tot / max(count, 1)
        per_th.append({"threshold": names[k], "count": count, "failed": zero, "iou": avg[0], "iocm": avg[1],
                       "directed_hd": avg[2] if want_hausdorff else None, "hd": avg[3] if want_hausdorff else None})
    best = max(per_th, key=lambda r: r["iocm"])
    return {"per_threshold": per_th, "best": best, "mean_average_precision": float(np.mean([r["iocm"] for r in per_th]))}


def print_report(res, frames=None, names=None, file=None):
    """The lines `evaluation.py --map` prints (per frame and threshold folder, then the summary)."""
    if frames is not None:
        for k in sorted(range(len(names)), key=lambda j: names[j]):
            for label, counts, _ in frames:
                iou, iocm = counts_to_iou(counts[k][0], counts[k][1], counts[k][2])
                print(f"IoU for {label}: {iou:.4f}\nIoCM for {label}: {iocm:.4f}", file=file)
    b = res["best"]
    print(f"mean average precision: {res['mean_average_precision']}", file=file)
    print(f"Best performing threshold was {b['threshold']}", file=file)
    if b["hd"] is None:
        print(f"IoU: {b['iou']}\nPrecision: {b['iocm']}\nHausdorff-Distance: not computed (--score_hausdorff)\n"
              "Directed Hausdorff-Distance: not computed (--score_hausdorff)", file=file)
    else:
        print(f"IoU: {b['iou']}\nPrecision: {b['iocm']}\nHausdorff-Distance: {b['hd']}\nDirected Hausdorff-Distance: {b['directed_hd']}",
              file=file)


def _read_gray(path):
    from PIL import Image
    return np.array(Image.open(path).convert("L"))


class BenchmarkScorer:
    """Scores an inference run against `<benchmark>/<video>/<frame>/{aff_left, aff_right, obj_left, obj_right}.png` as
    `evaluation.evaluate_folders(benchmark, predictions, calc_map=True, is_cropped=cropped, take_intersection=intersection)` would
    score the PNG tree inference.py writes, without the tree: add_batch() per evaluate() call (in the benchmark's sorted folder
    order, which is inference.iter_examples'), report() once at the end.

    Frame rules (evaluation.score_frame): a frame without [SEG] is skipped (no prediction folder would exist), as is one with no
    ground-truth plane at all, one whose ground-truth shape differs from the target shape ((855, 855), or the frame's own size when
    cropped), and, with intersection, one whose obj_<side>.png is missing or mis-sized for a hand that is written. Which hands are
    written is the taxonomy gate's decision and stays on the device: such a frame is scored anyway and dropped in report(), from the
    frame's argmax read back together with the counts.

    hausdorff: the kernel also writes the predicted union planes. True: they are read back per batch and
    `evaluation.calculate_hausdorff` runs on them in one worker thread (close() ends it). "device": one ops.contour_hausdorff call
    per batch walks them and the ground-truth union (built on the device from the uploaded planes) and measures the T pairs of every
    frame; the integers are read back with the counts, and no thread exists. The planes (T + 1 per frame, 0.7 MB each at 855 x 855)
    stay in HBM until report(): a frame whose result carries a flag (a contour of more than `max_vertices` vertices, or a kernel
    bound that no input should reach) is read back and recomputed by `evaluation.calculate_hausdorff` there, and counted in
    `host_walks`. Without hausdorff the two fields of the report are None.

    visualize: None, or a dict {"dir", "threshold" (one of thresholds, default 0.5), "caption" (default "Aff-Ex"), "examples"
    (default 20, 0 = all)}: `evaluation.py --visualize` on the tree the run would write at that
    threshold, drawn by the scoring call itself (haff_score_vis) from the very per-pixel decisions it counts. The first `examples`
    scored frames, in the benchmark's sorted order (the reference shuffles), get a canvas and an overlay record; after the batch's
    launch its canvases, its slice of the counts and the argmax of its frames with a missing object plane are read back in one copy,
    the captions are drawn (the IoU is that of the counts) and the PNGs written. A frame the rules above drop is neither drawn nor
    counted. add_batch then needs frames_u8, the frames as loaded (uint8 [H0, W0, 3] in HBM)."""

    def __init__(self, benchmark_dir, device, thresholds=postprocess.THRESHOLDS, names=None, cropped=False, intersection=False,
                 hausdorff=False, max_vertices=65536, visualize=None):
        self.benchmark_dir, self.device = benchmark_dir, torch.device(device)
        self.thresholds = tuple(thresholds)
        self.names = list(names) if names is not None else [str(t) for t in self.thresholds]
        assert len(self.names) == len(self.thresholds) and 1 <= len(self.thresholds) <= ops.SCORE_MAX_THRESHOLDS
        self.logit_ths = [postprocess.sigmoid_logit_threshold(t) for t in self.thresholds]
        if hausdorff not in (False, True, "device"):
            raise ValueError(f"hausdorff={hausdorff!r}: False, True (host thread) or 'device'")
        self.cropped, self.intersection, self.hausdorff = bool(cropped), bool(intersection), bool(hausdorff)
        self.hausdorff_device, self.max_vertices, self.host_walks = hausdorff == "device", int(max_vertices), 0
        self._labels, self._counts, self._gates, self._needs_gate, self._hd = [], [], [], [], []
        self._hd_results, self._hd_planes = [], []
        self._pool = None
        self.visualize, self.panels = None, []       # panels: (label, iou, path or None) of every frame drawn
        if visualize is not None:
            v = {"threshold": 0.5, "caption": "Aff-Ex", "examples": 20, **visualize}
            if v["threshold"] not in self.thresholds:
                raise ValueError(f"visualize threshold {v['threshold']}: one of {self.thresholds}")
            os.makedirs(v["dir"], exist_ok=True)
            v["t"] = self.thresholds.index(v["threshold"])
            v["left"] = int(v["examples"]) if int(v["examples"]) > 0 else float("inf")
            self.visualize, self._vis_tables = v, {}
        if self.hausdorff and not self.hausdorff_device:
            from concurrent.futures import ThreadPoolExecutor
            self._pool = ThreadPoolExecutor(max_workers=1, thread_name_prefix="haff-hausdorff")

    def close(self):
        if self._pool is not None:
            self._pool.shutdown(wait=True, cancel_futures=True)
            self._pool = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _frame(self, dir_name, folder_name, masks_left, masks_right, taxonomy, frame_hw):
        """The descriptor dict of one frame, or None when the frame rules skip it on the host's knowledge alone."""
        if taxonomy.numel() == 0:                              # no [SEG]: inference.py writes nothing
            return None
        hands = {}
        for side, masks in (("left", masks_left), ("right", masks_right)):
            if masks.shape[0] != 0:
                hands[side] = masks[0].float().contiguous()
        if not hands:
            return None
        target_hw = (int(frame_hw[0]), int(frame_hw[1])) if self.cropped else BENCHMARK_HW
        leaf = os.path.join(self.benchmark_dir, dir_name, folder_name)
        f = {"left": hands.get("left"), "right": hands.get("right"), "target_hw": target_hw,
             "taxonomy": taxonomy.reshape(-1).float().contiguous(), "gt_host": {}, "obj_missing": []}
        for side in ("left", "right"):
            p = os.path.join(leaf, f"aff_{side}.png")
            if os.path.exists(p):
                g = _read_gray(p)
                if g.shape != target_hw:
                    return None
                f["gt_host"][side] = g
                f[f"gt_{side}"] = ops.upload_pinned(g, self.device)
        if not f["gt_host"]:
            return None
        if self.intersection:
            for side in hands:
                p = os.path.join(leaf, f"obj_{side}.png")
                o = _read_gray(p) if os.path.exists(p) else None
                if o is None or o.shape != target_hw:
                    f["obj_missing"].append(side)              # skipped iff this hand is written: the gate decides
                else:
                    f[f"obj_{side}"] = ops.upload_pinned(o, self.device)
        return f

    def _vis_record(self, f, key, frame_u8):
        """The overlay record of one frame that is about to be scored (pack_vis's dict), with its canvas: [Hf, 2 Wf, 3] for the
        side-by-side panel, [Hf, Wf, 3] (the prediction overlay alone) with the caption "."."""
        from . import cvlite
        if frame_u8 is None or not frame_u8.is_cuda:
            raise RuntimeError("visualize needs frames_u8: the frames as loaded, uint8 [H0, W0, 3] in HBM")
        hf, wf = int(frame_u8.shape[0]), int(frame_u8.shape[1])
        hb, wb = f["target_hw"]
        row = col = None
        if (hf, wf) != (hb, wb):          # one table pair per distinct geometry, uploaded once
            if (hb, wb, hf, wf) not in self._vis_tables:
                self._vis_tables[hb, wb, hf, wf] = tuple(ops.upload_pinned(cvlite.nearest_indices(n, m).astype(np.int32), self.device)
                                                         for n, m in ((hf, hb), (wf, wb)))
            row, col = self._vis_tables[hb, wb, hf, wf]
        both = self.visualize["caption"] != "."
        canvas = torch.empty((hf, (2 if both else 1) * wf, 3), dtype=torch.uint8, device=self.device)
        return {"rgb": frame_u8.contiguous(), "row": row, "col": col, "t": self.visualize["t"], "canvas": canvas, "key": key,
                "out": (canvas[:, :wf], canvas[:, wf:]) if both else (None, canvas)}

    def _write_panels(self, frames, records, counts):
        """Behind the batch's launch: ONE device -> host copy of the canvases, the batch's counts and the argmax of its frames with
        a missing object plane; then the captions and the PNGs."""
        from . import evaluation
        v, T = self.visualize, len(self.thresholds)
        drawn = [f for f in frames if f.get("vis")]
        gates = [torch.argmax(f["taxonomy"]).to(torch.int32).reshape(1) for f in drawn if f["obj_missing"]]
        parts = [r["canvas"].reshape(-1) for r in records] + [torch.cat([counts.reshape(-1)] + gates).view(torch.uint8)]
        flat = torch.cat(parts).cpu().numpy()
        n_canvas = sum(r["canvas"].numel() for r in records)
        ints = flat[n_canvas:].view(np.int32)
        counts_host = ints[:len(frames) * T * 4].reshape(len(frames), T, 4)
        gate_vals = iter(ints[len(frames) * T * 4:].tolist())
        at = 0
        for i, f in enumerate(frames):
            if not f.get("vis"):
                continue
            r = records[f["vis"] - 1]
            canvas = flat[at:at + r["canvas"].numel()].reshape(tuple(r["canvas"].shape))
            at += r["canvas"].numel()
            if f["obj_missing"]:
                t = next(gate_vals)
                if any(t != (1 if side == "left" else 0) for side in f["obj_missing"]):
                    continue                                   # report() drops this frame: not drawn, not counted
            if v["left"] <= 0:
                continue
            v["left"] -= 1
            sub, leaf = r["key"]
            iou, _ = counts_to_iou(*counts_host[i][v["t"]][:3])
            wf = r["rgb"].shape[1]
            bench = canvas[:, :wf] if v["caption"] != "." else None
            path = evaluation.write_panel(v["dir"], sub, leaf, v["caption"], iou, bench, canvas[:, -wf:])
            self.panels.append((f["label"], iou, path))

    def add_batch(self, keys, masks_left, masks_right, taxonomies, frame_hws, frames_u8=None):
        """One evaluate() call: keys = [(dir_name, folder_name)], the three lists evaluate() returns, the frames' (H0, W0), and with
        visualize the frames themselves."""
        frames, records, sure = [], [], 0
        for b, (dir_name, folder_name) in enumerate(keys):
            f = self._frame(dir_name, folder_name, masks_left[b], masks_right[b], taxonomies[b], frame_hws[b])
            if f is None:
                continue
            if self.hausdorff:
                f["out"] = torch.empty((len(self.thresholds),) + f["target_hw"], dtype=torch.uint8, device=self.device)
            f["label"] = f"{dir_name}/{folder_name}"
            v = self.visualize
            if v is not None and sure < v["left"]:
                records.append(self._vis_record(f, (dir_name, folder_name), None if frames_u8 is None else frames_u8[b]))
                f["vis"] = len(records)
                sure += not f["obj_missing"]                   # a frame the gate may still drop does not use up the quota
            frames.append(f)
        if not frames:
            return
        counts = ops.score_masks(pack_frames(frames), self.logit_ths, self.device, **({"vis": pack_vis(records)} if records else {}))
        self._counts.append(counts.reshape(-1))
        if records:
            self._write_panels(frames, records, counts)
        for f in frames:
            self._labels.append(f["label"])
            self._needs_gate.append(f["obj_missing"])
            self._gates.append(torch.argmax(f["taxonomy"]).to(torch.int32).reshape(1) if f["obj_missing"] else None)
            if self.hausdorff and not self.hausdorff_device:
                g = f["gt_host"]
                bench = np.logical_or(g["left"] > 0, g["right"] > 0) if len(g) == 2 else next(iter(g.values())) > 0
                self._hd.append(self._pool.submit(_hausdorff_planes, bench, f["out"].cpu().numpy()))
        if self.hausdorff_device:
            self._hausdorff_device(frames)

    def _hausdorff_device(self, frames):
        """One ops.contour_hausdorff call over the batch, behind ops.score_masks in the same stream: per frame the ground-truth union
        and the T predicted unions the scoring kernel just wrote, paired (ground truth, threshold t)."""
        T = len(self.thresholds)
        planes, pairs = [], []
        for f in frames:
            gts = [f[k] > 0 for k in ("gt_left", "gt_right") if k in f]          # a missing hand counts as empty
            bench = (gts[0] | gts[1] if len(gts) == 2 else gts[0]).to(torch.uint8)
            base = len(planes)
            planes.append(bench)
            planes += [f["out"][t] for t in range(T)]
            pairs += [(base, base + 1 + t) for t in range(T)]
            self._hd_planes.append((bench, f["out"]))
        self._hd_results.append(ops.contour_hausdorff(planes, pairs, max_vertices=self.max_vertices).reshape(-1))

    def report(self, verbose=False, file=None):
        """The dict evaluation.evaluate_folders(..., calc_map=True) returns. ONE device -> host read: every frame's counts, and the
        argmax of the frames whose object plane was missing."""
        T = len(self.thresholds)
        if not self._labels:
            frames = []
        else:
            gates = [g for g in self._gates if g is not None]
            flat = torch.cat(self._counts + gates + self._hd_results).cpu().numpy().astype(np.int64)
            n = len(self._labels)
            counts = flat[:n * T * 4].reshape(n, T, 4)
            gate_vals = iter(flat[n * T * 4:n * T * 4 + len(gates)].tolist())
            if self.hausdorff_device:
                self._hd = self._device_distances(flat[n * T * 4 + len(gates):].reshape(n, T, 6))
            frames = []
            for i, label in enumerate(self._labels):
                if self._needs_gate[i]:
                    t = next(gate_vals)
                    if any(t != (1 if side == "left" else 0) for side in self._needs_gate[i]):
                        continue                               # a written hand without its object plane: score_frame returns None
                hd = None
                if self.hausdorff:
                    hd = self._hd[i] if self.hausdorff_device else self._hd[i].result()
                frames.append((label, counts[i], hd))
        res = report_from_frames(self.names, frames, self.hausdorff)
        if verbose:
            print_report(res, frames, self.names, file=file)
        return res


    def _device_distances(self, res):
        """Per frame the [T] (directed, symmetric) tuples evaluation.calculate_hausdorff returns, from the device's integers
        res [n, T, 6]: math.sqrt of an integer is scipy's value to the bit; no predicted contour gives the plane's diagonal, otherwise
        no ground-truth contour gives (0, 0). A flagged frame is walked on the host."""
        out = []
        self.host_walks = 0
        for i, label in enumerate(self._labels):
            bench, pred = self._hd_planes[i]
            flags = int(np.bitwise_or.reduce(res[i, :, 4]))
            if flags:
                if flags & ops.HAUSDORFF_FAULT:
                    print(f"warning: the device contour walk reported a fault on frame {label} (flags {flags:#x}); "
                          "its Hausdorff distances are recomputed on the host", file=sys.stderr)
                out.append(host_walk(self, lambda b, p: _hausdorff_planes(b > 0, p), bench, pred))
                continue
            h, w = bench.shape
            row = []
            for nb, npred, d_pb, d_bp, _, _ in res[i].tolist():
                if npred == 0:
                    d = float(np.sqrt(h ** 2 + w ** 2))
                    row.append((d, d))
                elif nb == 0:
                    row.append((0, 0))
                else:
                    row.append((math.sqrt(d_pb), math.sqrt(max(d_pb, d_bp))))
            out.append(row)
        return out


def _hausdorff_planes(bench_union, pred_planes):
    from . import evaluation
    return [evaluation.calculate_hausdorff(bench_union, pred_planes[t] > 0) for t in range(pred_planes.shape[0])]
