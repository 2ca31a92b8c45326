"""ActAffordance benchmark scoring — the harness AFTER the hot path.

Mirrors `ActAffordance/scripts/evaluation/calculate_iou.py`: walks `<benchmark>/<video>/<frame>/{aff_left,aff_right}.png`
against `<comparison>[/<threshold>]/<video>/<frame>/{aff_left,aff_right}.png` (what `inference.py:294-334` writes),
takes the union of both hands on each side (a missing hand counts as empty, :243-261), and reports IoU, IoCM
("precision": intersection over the predicted area), Hausdorff and directed Hausdorff averages; with `--map` the
threshold folders are swept and the best-IoCM one is reported together with the mean over thresholds (:321-343).

Exact restatements: `calculate_iou` (:26-41), `calculate_iocm` (:97-114), the union / missing-hand rules, the
averaging and threshold selection, the CLI flags, and `calculate_hausdorff` (:9-24) on the point set the reference uses: the
vertices of the FIRST external contour OpenCV returns (`findContours(RETR_EXTERNAL, CHAIN_APPROX_SIMPLE)[0][0]`, first contour
only) — through `cvlite.find_contours_external`, a restatement of OpenCV's border follower (no cv2 in this image: fixtures
hand-derived, tests/test_cvlite_cpu.py; parity with cv2 itself unpinned). Approximation: the reference resizes predictions with
`cv2.resize` (bilinear, no antialias -> here `F.interpolate(bilinear, align_corners=False)`).

`--visualize` (:43-95, :272-301) is the host route of the overlay panels and the yardstick of the device route (`inference.py
--visualize`, scoring.BenchmarkScorer(visualize=), csrc/mask_score.hip): `create_overlay` is the two `cv2.addWeighted` calls in numpy
fp32 with `np.rint` on `cvlite.resize_nearest`, `draw_captions` the three texts. Deviations, stated: the frames are taken in sorted
order (the reference shuffles the videos), the hard-coded clip of one frame (:297-298) is left out, and --visualize together with
--map, --only or --intersection is refused (the reference ignores those flags in that mode). Glyph pixels depend on the installed
Pillow's default font and are unpinned against the reference's.
"""
import argparse
import os

import numpy as np


def calculate_iou(mask1, mask2):
    """calculate_iou.py:26-41 — None when either mask is the empty placeholder, 0 when the union is empty."""
    if mask1.size == 0 or mask2.size == 0:
        return None
    inter = np.logical_and(mask1, mask2).sum()
    union = np.logical_or(mask1, mask2).sum()
    return float(inter) / float(union) if union != 0 else 0.0


def calculate_iocm(benchmark_mask, comparison_mask):
    """calculate_iou.py:97-114 — intersection over the comparison (predicted) area."""
    if comparison_mask.size == 0 or benchmark_mask.size == 0:
        return None
    inter = np.logical_and(benchmark_mask, comparison_mask).sum()
    area = comparison_mask.sum()
    return float(inter) / float(area) if area != 0 else 0.0


def calculate_hausdorff(mask1, mask2):
    """calculate_iou.py:9-24: (directed mask2 -> mask1, symmetric) Hausdorff distance between the CHAIN_APPROX_SIMPLE vertices of
    the first external contour of each mask. Empty prediction (mask2) -> the image diagonal for both; empty benchmark -> 0."""
    from scipy.spatial.distance import directed_hausdorff
    from . import cvlite
    shp = mask1.shape
    c1 = cvlite.find_contours_external(np.asarray(mask1).astype(np.uint8))
    c2 = cvlite.find_contours_external(np.asarray(mask2).astype(np.uint8))
    if len(c2) == 0:
        d = float(np.sqrt(shp[0] ** 2 + shp[1] ** 2))
        return d, d
    if len(c1) == 0:
        return 0, 0
    p1 = c1[0].reshape(-1, 2).astype(np.float64)      # np.vstack(contours[0]).squeeze(), a single point kept 2-D
    p2 = c2[0].reshape(-1, 2).astype(np.float64)
    d21 = directed_hausdorff(p2, p1)[0]
    return float(d21), float(max(directed_hausdorff(p1, p2)[0], d21))


def _read_gray(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("L"))


def _resize_bilinear(img_u8, size_wh):
    """cv2.resize(img, (w, h)) stand-in: bilinear on half-pixel centres, no antialiasing."""
    import torch
    import torch.nn.functional as F
    w, h = size_wh
    if img_u8.shape == (h, w):
        return img_u8
    t = torch.from_numpy(img_u8.astype(np.float32))[None, None]
    return F.interpolate(t, size=(h, w), mode="bilinear", align_corners=False)[0, 0].round().clamp(0, 255).numpy().astype(np.uint8)


def _load_hands(bench_dir, comp_dir, orig_shape_wh, take_intersection=False):
    """The four boolean masks of one leaf folder, (benchmark left, right, comparison left, right), each the empty (0, 0) placeholder
    where its file is missing; the comparison masks resized to orig_shape_wh and, with take_intersection, ANDed with the annotated
    object mask. None when an object mask is missing or mis-sized: the frame is skipped."""
    empty = np.zeros((0, 0))
    b_left = b_right = c_left = c_right = empty
    p = os.path.join(bench_dir, "aff_left.png")
    if os.path.exists(p):
        b_left = _read_gray(p) > 0
    p = os.path.join(bench_dir, "aff_right.png")
    if os.path.exists(p):
        b_right = _read_gray(p) > 0
    for side in ("left", "right"):
        p = os.path.join(comp_dir, f"aff_{side}.png")
        if not os.path.exists(p):
            continue
        m = _resize_bilinear(_read_gray(p), orig_shape_wh)
        if take_intersection:  # calculate_iou.py:207-215 — restrict the prediction to the annotated object mask
            op = os.path.join(bench_dir, f"obj_{side}.png")
            if not os.path.exists(op):
                return None
            obj = _read_gray(op)
            if obj.shape != m.shape:
                return None
            m = np.bitwise_and(m, obj)
        if side == "left":
            c_left = m > 0
        else:
            c_right = m > 0
    return b_left, b_right, c_left, c_right


def score_frame(bench_dir, comp_dir, orig_shape_wh, take_intersection=False):
    """One leaf folder: (iou, iocm, directed_hd, hd) of the two-hand unions, or None when the frame is skipped."""
    hands = _load_hands(bench_dir, comp_dir, orig_shape_wh, take_intersection)
    if hands is None:
        return None
    b_left, b_right, c_left, c_right = hands

    def union(a, b):
        if a.size and b.size:
            return np.logical_or(a, b)
        return a if a.size else b
    bench_union, comp_union = union(b_left, b_right), union(c_left, c_right)
    if bench_union.size and comp_union.size and bench_union.shape != comp_union.shape:
        return None   # (the reference's np.logical_and raises here: e.g. --cropped with full-resolution masks; the frame is skipped)
    iou, iocm = calculate_iou(bench_union, comp_union), calculate_iocm(bench_union, comp_union)
    if iou is None or iocm is None:
        return None
    dhd, hd = calculate_hausdorff(bench_union, comp_union)
    return iou, iocm, dhd, hd


def evaluate_folders(benchmark_folder, comparison_folder, only=None, calc_map=False, is_cropped=False,
                     take_intersection=False, n_examples=float("inf"), verbose=True):
    """calculate_iou.py:117-343 without the overlays. Returns a dict with the per-threshold averages and the pick."""
    subfolders = sorted(os.listdir(benchmark_folder))
    if only == "ego":
        subfolders = [s for s in subfolders if not s.startswith("P")]
    if only == "epic":
        subfolders = [s for s in subfolders if s.startswith("P")]
    thresholds = sorted(os.listdir(comparison_folder)) if calc_map else ["."]
    per_th = []
    for th in thresholds:
        th_dir = os.path.join(comparison_folder, th)
        tot = np.zeros(4)
        count = zero = 0
        for sub in subfolders:
            bsub, csub = os.path.join(benchmark_folder, sub), os.path.join(th_dir, sub)
            if not (os.path.isdir(bsub) and os.path.isdir(csub)):
                continue
            for leaf in sorted(os.listdir(bsub)):
                bleaf, cleaf = os.path.join(bsub, leaf), os.path.join(csub, leaf)
                if not (os.path.isdir(bleaf) and os.path.isdir(cleaf)):
                    continue
                inpaint = os.path.join(bleaf, "inpainting.png")
                if not os.path.exists(inpaint):
                    continue
                shape_wh = (855, 855)                      # calculate_iou.py:139: the uncropped benchmark resolution
                if is_cropped:
                    from PIL import Image
                    shape_wh = Image.open(inpaint).size     # (w, h)
                res = score_frame(bleaf, cleaf, shape_wh, take_intersection)
                if res is None:
                    continue
                tot += np.asarray(res)
                zero += int(res[0] == 0 and res[1] == 0)
                count += 1
                if verbose:
                    print(f"IoU for {sub}/{leaf}: {res[0]:.4f}\nIoCM for {sub}/{leaf}: {res[1]:.4f}")
                if count >= n_examples:
                    break
        avg = tot / max(count, 1)
        per_th.append({"threshold": th, "count": count, "failed": zero, "iou": avg[0], "iocm": avg[1],
                       "directed_hd": avg[2], "hd": avg[3]})
    best = max(per_th, key=lambda r: r["iocm"])
    out = {"per_threshold": per_th, "best": best}
    if calc_map:
        out["mean_average_precision"] = float(np.mean([r["iocm"] for r in per_th]))
    return out


OVERLAY_LEFT_RGB, OVERLAY_RIGHT_RGB = (255, 0, 0), (0, 255, 0)   # :76-78 in RGB: red, and green (the comment there says blue)


def _add_weighted(a, alpha, b, beta, gamma):
    """cv2.addWeighted on uint8: fp32 a * alpha + b * beta + gamma, rounded half to even, saturated."""
    v = a.astype(np.float32) * np.float32(alpha) + b.astype(np.float32) * np.float32(beta) + np.float32(gamma)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def create_overlay(frame_rgb, left, right, alpha=0.5, beta=0.5, gamma=0):
    """calculate_iou.py:60-85 on an RGB frame uint8 [Hf, Wf, 3]: the two masks (boolean, any one size; None = all off) are resized to
    the frame by cv2.INTER_NEAREST, coloured red (left) and green (right), and blended in twice: frame * alpha + left * beta + gamma,
    then that * 1 + right * beta + gamma. Both blends always run: a missing hand still halves the frame. Returns uint8 [Hf, Wf, 3]."""
    from . import cvlite
    frame_rgb = np.asarray(frame_rgb)
    hf, wf = frame_rgb.shape[:2]
    layers = []
    for mask, rgb in ((left, OVERLAY_LEFT_RGB), (right, OVERLAY_RIGHT_RGB)):
        plane = np.zeros((hf, wf), np.uint8)
        if mask is not None and np.asarray(mask).size:
            plane = cvlite.resize_nearest(np.uint8(np.asarray(mask) * 255), (wf, hf))
        layers.append((plane[:, :, None] > 0) * np.asarray(rgb, np.uint8)[None, None, :])
    combined = _add_weighted(frame_rgb, alpha, layers[0], beta, gamma)
    return _add_weighted(combined, 1, layers[1], beta, gamma)


def draw_captions(canvas_rgb, texts):
    """The captions of :86-92 and :289-291 on a finished panel: canvas_rgb uint8 [H, W, 3]; texts = (text, x) pairs, x >= 0 the left
    edge, x < 0 the right edge the text ends 10 pixels before, counted from the canvas's left as -x (a panel's right edge). White,
    ImageFont.load_default(), at y = 10; the width is font.getbbox(text)[2]. Returns the PIL image."""
    from PIL import Image, ImageDraw, ImageFont
    img = Image.fromarray(np.ascontiguousarray(canvas_rgb))
    draw = ImageDraw.Draw(img)
    font = ImageFont.load_default()
    for text, x in texts:
        if x < 0:
            x = -x - font.getbbox(text)[2] - 10
        draw.text((x, 10), text, fill="white", font=font)
    return img


def panel_captions(label, caption, iou, frame_w):
    """The three texts of a side-by-side panel: the frame's label on the benchmark half, the caption on the prediction half, the IoU."""
    return [(label, -frame_w), (caption, -2 * frame_w), (f"IoU: {iou:.4f}", 10)]


def files_filter(files_folder):
    """calculate_iou.py:152-175: the (video, frame) pairs named by the files of --files_folder, `<video>_<frame>.<ext>` where the
    video may hold one underscore. A frame passes when its FIRST listing names its video."""
    vids, frames = [], []
    for name in os.listdir(files_folder):
        parts = name.split("_")
        if len(parts) > 2:
            vids.append(parts[0] + "_" + parts[1])
            frames.append(parts[2].split(".")[0])
        else:
            vids.append(parts[0])
            frames.append(parts[1].split(".")[0])
    return lambda sub, leaf: leaf in frames and vids[frames.index(leaf)] == sub


def panel_path(visualize_dir, sub, leaf, caption):
    return os.path.join(visualize_dir, f"{sub}_{leaf}_concatenated.png" if caption != "." else f"{sub}_{leaf}.png")


def write_panel(visualize_dir, sub, leaf, caption, iou, bench_overlay, pred_overlay, keep_all=False):
    """:272-301 from finished overlays (uint8 [Hf, Wf, 3]; bench_overlay unused with the caption "."): the captioned side-by-side panel,
    or with the caption "." the prediction overlay alone, and only when the IoU exceeds 0.2 or keep_all (--files_folder). Returns the
    path written, or None."""
    path = panel_path(visualize_dir, sub, leaf, caption)
    if caption != ".":
        canvas = np.concatenate([bench_overlay, pred_overlay], axis=1)
        draw_captions(canvas, panel_captions(f"{sub}/{leaf}", caption, iou, pred_overlay.shape[1])).save(path)
    elif iou > 0.2 or keep_all:
        draw_captions(pred_overlay, []).save(path)
    else:
        return None
    return path


def _hand_masks(bench_dir, comp_dir, orig_shape_wh):
    """score_frame's masks of one leaf folder as :237-255 leaves them for the overlays (a missing hand all off) and the two unions,
    or None where score_frame skips the frame."""
    b_left, b_right, c_left, c_right = _load_hands(bench_dir, comp_dir, orig_shape_wh)
    bench, comp = [m for m in (b_left, b_right) if m.size], [m for m in (c_left, c_right) if m.size]
    if not bench or not comp or any(m.shape != comp[0].shape for m in bench):
        return None
    masks = {("b", "left"): b_left, ("b", "right"): b_right, ("c", "left"): c_left, ("c", "right"): c_right}
    for (who, side), m in list(masks.items()):
        if not m.size:
            masks[who, side] = np.zeros_like(bench[0] if who == "b" else comp[0])
    return masks, np.logical_or.reduce(bench), np.logical_or.reduce(comp)


def visualize_folders(benchmark_folder, comparison_folder, visualize_dir, caption="Aff-Ex", n_examples=20, files_folder=None,
                      is_cropped=False, verbose=True):
    """calculate_iou.py --visualize (:117-307 with visualize=True): the first n_examples scored frames of comparison_folder, in sorted
    order, as panels under visualize_dir. Returns [(label, iou, path or None)]."""
    os.makedirs(visualize_dir, exist_ok=True)
    keep = files_filter(files_folder) if files_folder else None
    done = []
    for sub in sorted(os.listdir(benchmark_folder)):
        bsub, csub = os.path.join(benchmark_folder, sub), os.path.join(comparison_folder, sub)
        if not (os.path.isdir(bsub) and os.path.isdir(csub)):
            continue
        for leaf in sorted(os.listdir(bsub)):
            bleaf, cleaf = os.path.join(bsub, leaf), os.path.join(csub, leaf)
            inpaint = os.path.join(bleaf, "inpainting.png")
            if not (os.path.isdir(bleaf) and os.path.isdir(cleaf) and os.path.exists(inpaint)):
                continue
            if keep is not None and not keep(sub, leaf):
                continue
            from PIL import Image
            frame = np.asarray(Image.open(inpaint).convert("RGB"))
            found = _hand_masks(bleaf, cleaf, (frame.shape[1], frame.shape[0]) if is_cropped else (855, 855))
            if found is None:
                continue
            masks, bench_union, comp_union = found
            iou, iocm = calculate_iou(bench_union, comp_union), calculate_iocm(bench_union, comp_union)
            if verbose:
                print(f"IoU for {sub}/{leaf}: {iou:.4f}\nIoCM for {sub}/{leaf}: {iocm:.4f}")
            bench_overlay = create_overlay(frame, masks["b", "left"], masks["b", "right"]) if caption != "." else None
            path = write_panel(visualize_dir, sub, leaf, caption, iou, bench_overlay,
                               create_overlay(frame, masks["c", "left"], masks["c", "right"]), keep_all=bool(files_folder))
            done.append((f"{sub}/{leaf}", iou, path))
            if len(done) >= n_examples:
                return done
    return done


def main(argv=None):
    ap = argparse.ArgumentParser(description="IoU / IoCM / Hausdorff between benchmark and prediction folders")
    ap.add_argument("--benchmark_folder", type=str, default="../../data/cropped")
    ap.add_argument("--comparison_folder", type=str, required=True)
    ap.add_argument("--num-examples", type=int, default=None)
    ap.add_argument("--only", default=None)
    ap.add_argument("--map", default=None, action="store_true")
    ap.add_argument("--cropped", default=None, action="store_true")
    ap.add_argument("--intersection", default=None, action="store_true")
    ap.add_argument("--visualize", action="store_true", help="write overlay panels of the first --num-examples (default 20) scored frames")
    ap.add_argument("--visualize-dir", type=str, default="./visualizations_new")
    ap.add_argument("--caption", type=str, default="Aff-Ex", help='"." writes the prediction overlay alone, for frames above IoU 0.2')
    ap.add_argument("--files_folder", type=str, default=None, help="with --visualize: only the frames its file names list")
    args = ap.parse_args(argv)
    if args.visualize:
        for flag in ("map", "only", "intersection"):
            if getattr(args, flag):
                raise SystemExit(f"--visualize draws one prediction folder as it is: --{flag} does not apply to it")
        return visualize_folders(args.benchmark_folder, args.comparison_folder, args.visualize_dir, caption=args.caption,
                                 n_examples=20 if args.num_examples is None else args.num_examples, files_folder=args.files_folder,
                                 is_cropped=bool(args.cropped))
    res = evaluate_folders(args.benchmark_folder, args.comparison_folder, only=args.only, calc_map=bool(args.map),
                           is_cropped=bool(args.cropped), take_intersection=bool(args.intersection),
                           n_examples=args.num_examples or float("inf"))
    b = res["best"]
    if not args.map:
        print(f"Total Failed Predictions: {b['failed']}")
        print(f"Total Averaged IoU: {b['iou']}")
        print(f"Total Averaged IoCM: {b['iocm']}")
        print(f"Total Averaged Hausdorff Distance: {b['hd']}")
        print(f"Total Averaged Directed Hausdorff Distance: {b['directed_hd']}")
    else:
        print(f"mean average precision: {res['mean_average_precision']}")
        print(f"Best performing threshold was {b['threshold']}")
        print(f"IoU: {b['iou']}\nPrecision: {b['iocm']}\nHausdorff-Distance: {b['hd']}\nDirected Hausdorff-Distance: {b['directed_hd']}")
    return res


if __name__ == "__main__":
    main()
