"""Brute-force restatement of the overlay panels (calculate_iou.py:43-95 as csrc/mask_score.hip's score_vis_kernel draws them),
independent of evaluation.py and cvlite.py: the nearest-index rule in scalar Python doubles, the two cv2.addWeighted blends as a
table built from scalar fp32 arithmetic and Python's round (half to even), the layer bits from score_ref.resample_on / gate.

Per frame pixel (y, x): the target pixel (row[y], col[x]); a hand's prediction layer is on where the scoring rule turns it on at the
drawn threshold (gate, resample, obj AND), its benchmark layer where gt > 0; per channel byte = blend(blend(frame, alpha0, L, beta0),
alpha1, R, beta1), each blend a * alpha + b * beta + gamma in fp32, rounded half to even and saturated to 0..255.
"""
import math

import numpy as np

import score_ref as R

ALPHA, BETA, GAMMA = (0.5, 1.0), (0.5, 0.5), 0.0
COLORS = ((255, 0, 0), (0, 255, 0))          # RGB: left red, right green


def nearest_index(n_dst, n_src):
    """cv2.INTER_NEAREST along one axis: min(floor(x * ifx), n_src - 1), ifx = 1. / (n_dst / n_src) in doubles, one x at a time."""
    ifx = 1.0 / (float(n_dst) / float(n_src))
    return [min(int(math.floor(x * ifx)), n_src - 1) for x in range(n_dst)]


def blend_byte(a, alpha, b, beta, gamma):
    """One cv2.addWeighted output byte: fp32 products and sums one at a time, round half to even, saturate."""
    f = np.float32
    v = f(f(f(a) * f(alpha)) + f(f(b) * f(beta))) + f(gamma)
    r = round(float(f(v)))                    # Python's round: half to even, exact on a double that holds an fp32
    return max(0, min(255, r))


def blend_table(channel, alpha=ALPHA, beta=BETA, gamma=GAMMA, colors=COLORS):
    """uint8 [256, 2, 2]: the output byte of one channel for every frame byte and (left on, right on)."""
    t = np.zeros((256, 2, 2), np.uint8)
    for v in range(256):
        for left in (0, 1):
            t1 = blend_byte(v, alpha[0], colors[0][channel] if left else 0, beta[0], gamma)
            for right in (0, 1):
                t[v, left, right] = blend_byte(t1, alpha[1], colors[1][channel] if right else 0, beta[1], gamma)
    return t


def overlay(frame_rgb, left, right, alpha=ALPHA, beta=BETA, gamma=GAMMA, colors=COLORS):
    """uint8 [Hf, Wf, 3]: left / right are boolean planes on one grid (or None: all off), taken to the frame by the nearest rule."""
    frame_rgb = np.asarray(frame_rgb)
    hf, wf = frame_rgb.shape[:2]
    bits = []
    for plane in (left, right):
        if plane is None:
            bits.append(np.zeros((hf, wf), np.int64))
            continue
        plane = np.asarray(plane).astype(bool)
        rows, cols = nearest_index(hf, plane.shape[0]), nearest_index(wf, plane.shape[1])
        bits.append(plane[np.asarray(rows)][:, np.asarray(cols)].astype(np.int64))
    out = np.zeros((hf, wf, 3), np.uint8)
    for c in range(3):
        out[:, :, c] = blend_table(c, alpha, beta, gamma, colors)[frame_rgb[:, :, c], bits[0], bits[1]]
    return out


def hand_bits(f, th):
    """(prediction left, right; benchmark left, right) of a frame dict (left / right logits, taxonomy, gt_*, obj_*, target_hw) on the
    target grid at LOGIT threshold th, by the scoring rule: boolean [Hb, Wb] each."""
    hb, wb = f["target_hw"]
    pred = []
    for logits, is_open, obj in zip((f["left"], f["right"]), R.gate(f["taxonomy"]), (f["obj_left"], f["obj_right"])):
        m = np.zeros((hb, wb), bool)
        if logits is not None and is_open:
            with np.errstate(invalid="ignore"):
                m = R.resample_on(np.asarray(logits, dtype=np.float32) > np.float32(th), (hb, wb))
            if obj is not None:
                m = m & (np.asarray(obj) > 0)
        pred.append(m)
    bench = [np.zeros((hb, wb), bool) if g is None else np.asarray(g) > 0 for g in (f["gt_left"], f["gt_right"])]
    return pred, bench


def panels(f, th, frame_rgb, **weights):
    """(benchmark overlay, prediction overlay) uint8 [Hf, Wf, 3] of one scored frame."""
    pred, bench = hand_bits(f, th)
    return overlay(frame_rgb, bench[0], bench[1], **weights), overlay(frame_rgb, pred[0], pred[1], **weights)
