"""numpy restatement of csrc/mask_score.hip (haff_score_masks) and of the scorer built on it: the integer resample rule, the
taxonomy gate, the AND / union rules, the four counts, and `score_tree`, shaped like evaluation.evaluate_folders(calc_map=True).

Rule per target pixel, hand and threshold: the bilinear resample (half-pixel centres, no antialiasing) of the 0/255 plane
`logit > th`, then `> 0`, in exact integers. Per axis num = max((2o+1) n_in - n_out, 0), i0 = min(num // 2 n_out, n_in - 1),
i1 = min(i0 + 1, n_in - 1), w1 = num mod 2 n_out (0 once i0 is clamped), w0 = 2 n_out - w1; S = sum of wy wx [tap on];
on iff 510 S > 4 Hb Wb (the resampled byte is round-half-even(255 S / 4 Hb Wb), and 0.5 rounds to 0).
"""
import ctypes
import os

import numpy as np


def axis_taps(n_in, n_out):
    o = np.arange(n_out, dtype=np.int64)
    num = np.maximum((2 * o + 1) * n_in - n_out, 0)
    den = 2 * n_out
    q = num // den
    i0 = np.minimum(q, n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    w1 = np.where(q >= n_in - 1, 0, num % den)
    return i0, i1, den - w1, w1


def coverage(bits, target_hw):
    """S [Hb, Wb] int64 of a boolean source plane: sum over the four taps of wy wx [tap on]; the full weight is 4 Hb Wb."""
    bits = np.asarray(bits).astype(np.int64)
    hb, wb = target_hw
    y0, y1, wy0, wy1 = axis_taps(bits.shape[0], hb)
    x0, x1, wx0, wx1 = axis_taps(bits.shape[1], wb)
    s = (wy0[:, None] * wx0[None]) * bits[y0][:, x0] + (wy0[:, None] * wx1[None]) * bits[y0][:, x1]
    s += (wy1[:, None] * wx0[None]) * bits[y1][:, x0] + (wy1[:, None] * wx1[None]) * bits[y1][:, x1]
    return s


def resample_on(bits, target_hw):
    """bool [Hb, Wb]: `cv2.resize(255 * bits, target) > 0` by the exact rule."""
    hb, wb = target_hw
    return 510 * coverage(bits, target_hw) > 4 * hb * wb


def near_tie(bits, target_hw):
    """bool [Hb, Wb]: pixels whose exact resampled value 255 S / (4 Hb Wb) lies within 1530 max(Hs, Ws) 2^-23 of the tie at 0.5 —
    a bound on what fp32 source coordinates (a few ulp of a coordinate below max(Hs, Ws)) can move the value by."""
    hb, wb = target_hw
    v = 255.0 * coverage(bits, target_hw).astype(np.float64) / (4.0 * hb * wb)
    return np.abs(v - 0.5) <= 1530.0 * max(np.asarray(bits).shape) * 2.0 ** -23


def gate(taxonomy):
    """(left open, right open) from the flattened taxonomy vector: first maximum by strict `>` (a NaN never wins, as in the kernel);
    index 1 blanks left, index 0 blanks right. None: both open."""
    if taxonomy is None:
        return True, True
    t = np.asarray(taxonomy, dtype=np.float32).reshape(-1)
    best, bv = 0, t[0]
    for c in range(1, t.size):
        if t[c] > bv:
            best, bv = c, t[c]
    return best != 1, best != 0


def score_frame(left, right, taxonomy, gt_left, gt_right, obj_left, obj_right, thresholds, target_hw):
    """One frame of haff_score_masks: (counts int64 [T, 4] = intersection, union, predicted area, ground-truth area;
    unions uint8 [T, Hb, Wb] of 0/1). left / right: fp32 [Hs, Ws] logits or None; gt / obj: uint8 [Hb, Wb] or None."""
    hb, wb = target_hw
    open_l, open_r = gate(taxonomy)
    gt = np.zeros((hb, wb), bool)
    for g in (gt_left, gt_right):
        if g is not None:
            gt |= np.asarray(g) > 0
    counts = np.zeros((len(thresholds), 4), np.int64)
    unions = np.zeros((len(thresholds), hb, wb), np.uint8)
    for k, th in enumerate(thresholds):
        pred = np.zeros((hb, wb), bool)
        for logits, is_open, obj in ((left, open_l, obj_left), (right, open_r, obj_right)):
            if logits is None or not is_open:
                continue
            with np.errstate(invalid="ignore"):
                m = resample_on(np.asarray(logits, dtype=np.float32) > np.float32(th), target_hw)
            if obj is not None:
                m &= np.asarray(obj) > 0
            pred |= m
        unions[k] = pred
        counts[k] = ((pred & gt).sum(), (pred | gt).sum(), pred.sum(), gt.sum())
    return counts, unions


def iou_iocm(counts_row):
    inter, union, area = (int(v) for v in counts_row[:3])
    return (float(inter) / float(union) if union != 0 else 0.0), (float(inter) / float(area) if area != 0 else 0.0)


def _gray(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("L"))


def score_tree(benchmark_folder, comparison_folder, is_cropped=False, take_intersection=False, hausdorff=True):
    """evaluation.evaluate_folders(benchmark, comparison, calc_map=True, ...) with the exact resample rule in place of
    `_resize_bilinear(...) > 0`. Same walk, same skips, same accumulation order, same dict; the extra key "frames" lists, per
    threshold folder, (label, counts [4], near-tie pixel count) of every scored frame. hausdorff False: the two fields are None."""
    from PIL import Image
    from haff import evaluation
    subfolders = sorted(os.listdir(benchmark_folder))
    per_th, frames_out = [], {}
    for th in sorted(os.listdir(comparison_folder)):
        tot = np.zeros(4)
        count = zero = 0
        frames_out[th] = []
        for sub in subfolders:
            bsub, csub = os.path.join(benchmark_folder, sub), os.path.join(comparison_folder, th, sub)
            if not (os.path.isdir(bsub) and os.path.isdir(csub)):
                continue
            for leaf in sorted(os.listdir(bsub)):
                bleaf, cleaf = os.path.join(bsub, leaf), os.path.join(csub, leaf)
                inpaint = os.path.join(bleaf, "inpainting.png")
                if not (os.path.isdir(bleaf) and os.path.isdir(cleaf) and os.path.exists(inpaint)):
                    continue
                target_hw = (855, 855)
                if is_cropped:
                    w, h = Image.open(inpaint).size
                    target_hw = (h, w)
                gts = {s: _gray(os.path.join(bleaf, f"aff_{s}.png")) for s in ("left", "right")
                       if os.path.exists(os.path.join(bleaf, f"aff_{s}.png"))}
                preds = {s: _gray(os.path.join(cleaf, f"aff_{s}.png")) for s in ("left", "right")
                         if os.path.exists(os.path.join(cleaf, f"aff_{s}.png"))}
                if not gts or not preds or any(g.shape != target_hw for g in gts.values()):
                    continue
                objs, skip = {}, False
                if take_intersection:
                    for s in preds:
                        op = os.path.join(bleaf, f"obj_{s}.png")
                        if not os.path.exists(op) or _gray(op).shape != target_hw:
                            skip = True
                        else:
                            objs[s] = _gray(op)
                if skip:
                    continue
                pred = np.zeros(target_hw, bool)
                ties = 0
                for s, p in preds.items():
                    m = resample_on(p > 0, target_hw)
                    ties += int(near_tie(p > 0, target_hw).sum())
                    if s in objs:
                        m &= objs[s] > 0
                    pred |= m
                gt = np.zeros(target_hw, bool)
                for g in gts.values():
                    gt |= g > 0
                c = np.array([(pred & gt).sum(), (pred | gt).sum(), pred.sum(), gt.sum()], np.int64)
                iou, iocm = iou_iocm(c)
                dhd, hd = evaluation.calculate_hausdorff(gt, pred) if hausdorff else (0.0, 0.0)
                tot += np.asarray((iou, iocm, dhd, hd))
                zero += int(iou == 0 and iocm == 0)
                count += 1
                frames_out[th].append((f"{sub}/{leaf}", c, ties))
        avg = tot / max(count, 1)
        per_th.append({"threshold": th, "count": count, "failed": zero, "iou": avg[0], "iocm": avg[1],
                       "directed_hd": avg[2] if hausdorff else None, "hd": avg[3] if hausdorff else None})
    best = max(per_th, key=lambda r: r["iocm"])
    return {"per_threshold": per_th, "best": best, "mean_average_precision": float(np.mean([r["iocm"] for r in per_th])),
            "frames": frames_out}


# ---- haff_score_masks' host refusals (nothing is launched: the device pointers below are never dereferenced) ----

def descriptor_table(**over):
    """One descriptor (haff_score_frame as 16 int64 words) with fake, aligned, never-dereferenced device pointers."""
    fake = 0x10000
    f = {"left": fake, "right": fake + 0x4000, "tax": fake + 0x8000, "gt": (fake + 0x9001, 0), "obj": (0, fake + 0xA003),
         "out": 0, "hs": 5, "ws": 7, "hb": 13, "wb": 11, "n_tax": 4, "gt_hw": ((13, 11), (0, 0)), "obj_hw": ((0, 0), (13, 11))}
    f.update(over)
    t = np.zeros((1, 16), np.int64)
    t[0, :8] = [f["left"], f["right"], f["tax"], f["gt"][0], f["gt"][1], f["obj"][0], f["obj"][1], f["out"]]
    t.view(np.int32).reshape(1, 32)[0, 16:29] = [f["hs"], f["ws"], f["hb"], f["wb"], f["n_tax"], *f["gt_hw"][0], *f["gt_hw"][1],
                                                 *f["obj_hw"][0], *f["obj_hw"][1]]
    return t


def score_refusals(lib):
    """Every host refusal of haff_score_masks -> its error code."""
    th = (ctypes.c_float * 9)(*([0.0] * 9))
    thp = ctypes.cast(th, ctypes.c_void_p)
    fake_dev, counts = 0x20000, 0x30000

    def call(table, n_th=1, n=1, dev=fake_dev, cnt=counts, ths=thp, host=None):
        return int(lib.haff_score_masks(table.ctypes.data if host is None else host, dev, n, ths, n_th, cnt, None))
    ok = descriptor_table()
    got = {
        "n_th 0": call(ok, n_th=0), "n_th 9": call(ok, n_th=9), "n_th -1": call(ok, n_th=-1),
        "no frames": call(ok, n=0), "too many frames": call(ok, n=65536),
        "null table": call(ok, host=0), "null device table": call(ok, dev=0), "null counts": call(ok, cnt=0),
        "null thresholds": call(ok, ths=None),
        "misaligned device table": call(ok, dev=fake_dev + 4), "misaligned host table": call(ok, host=ok.ctypes.data + 4),
        "misaligned counts": call(ok, cnt=counts + 2),
        "misaligned left": call(descriptor_table(left=0x10002)), "misaligned right": call(descriptor_table(right=0x14001)),
        "misaligned taxonomy": call(descriptor_table(tax=0x18003)),
        "gt rows": call(descriptor_table(gt_hw=((12, 11), (0, 0)))), "gt columns": call(descriptor_table(gt_hw=((13, 12), (0, 0)))),
        "obj shape": call(descriptor_table(obj_hw=((0, 0), (11, 13)))),
        "gt right shape": call(descriptor_table(gt=(0x19001, 0x1B000), gt_hw=((13, 11), (13, 10)))),
        "zero side": call(descriptor_table(hs=0)), "negative side": call(descriptor_table(wb=-3, gt=(0, 0), obj=(0, 0))),
        "n_tax 0": call(descriptor_table(n_tax=0)), "n_tax 1025": call(descriptor_table(n_tax=1025)),
    }
    big = {f"{k} 4097": call(descriptor_table(**{k: 4097, "gt": (0, 0), "obj": (0, 0)})) for k in ("hs", "ws", "hb", "wb")}
    return got, big
