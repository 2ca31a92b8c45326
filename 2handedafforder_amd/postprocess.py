"""Output gating + thresholds of the reference's CLIs (row a15) on the device.

  inference.py:276-334 : argmax(taxonomy) != 1 -> emit left, != 0 -> emit right; per hand
                         `sigmoid(mask) > th` for th in (.1, .2, .3, .5, .7) -> 0/255 planes (cv2.imwrite PNGs)
  chat.py:226-253      : `mask > 0`; a blanked hand is still written (all zeros); planes are written as mask*100

Byte work, so the bar is bit-exact. `sigmoid(m) > th` is evaluated by the reference in fp32 (torch.sigmoid on the
fp32 mask, numpy compare against float32(th)); fp32 sigmoid is monotone, so the rule equals `m > x*(th)` for ONE fp32
constant x*(th) = the largest float with sigmoid_f32(x) <= float32(th). The constants below were found by bisection
over the fp32 ordering against torch.sigmoid (tests/test_abi_cpu.py re-derives them and checks the +-64-ulp
neighbourhood); the HIP kernel (haff_gate_threshold_masks) then only compares, reading each mask once for all
thresholds, and applies the taxonomy gate from the device-resident class probabilities.
"""
import struct

import torch

from . import ops

THRESHOLDS = (0.1, 0.2, 0.3, 0.5, 0.7)  # inference.py:197


def _f32_from_bits(b):
    return struct.unpack("<f", struct.pack("<I", b & 0xFFFFFFFF))[0]


def _ordered_to_f32(u):
    """inverse of the order-preserving map float32 -> uint32 (negative floats bit-flipped, positives offset)"""
    return _f32_from_bits(u ^ 0x80000000 if u & 0x80000000 else ~u)


def derive_sigmoid_logit_threshold(th):
    """Largest fp32 x with torch.sigmoid(float32(x)) <= float32(th), by bisection over the fp32 total order."""
    th32 = torch.tensor(th, dtype=torch.float32)

    def le(u):
        x = torch.full((16,), _ordered_to_f32(u), dtype=torch.float32)  # a full SIMD vector: the vectorised code path
        return bool((torch.sigmoid(x) <= th32).all())
    lo, hi = (~0xC2C80000) & 0xFFFFFFFF, 0x42C80000 | 0x80000000   # -100.0 .. +100.0 in ordered space
    assert le(lo) and not le(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if le(mid):
            lo = mid
        else:
            hi = mid
    return _ordered_to_f32(lo)


# x*(th) as fp32 bit patterns (derive_sigmoid_logit_threshold on torch 2.10 CPU; checked by tests/test_abi_cpu.py)
_LOGIT_TH_BITS = {0.1: 0xC00C9F54, 0.2: 0xBFB17218, 0.3: 0xBF58E882, 0.5: 0x33C00000, 0.7: 0x3F58E884}
_DERIVED = {}


def sigmoid_logit_threshold(th):
    """x*(th). Note x*(0.5) = 2^-23.4 > 0: sigmoid_f32 rounds to exactly 0.5 for 0 < m <= x*, so `sigmoid(m) > 0.5` is
    not `m > 0` — the chat rule (mask > 0) and the inference rule at th = 0.5 differ on those logits."""
    key = float(th)
    if key in _LOGIT_TH_BITS:
        return _f32_from_bits(_LOGIT_TH_BITS[key])
    if key not in _DERIVED:
        _DERIVED[key] = derive_sigmoid_logit_threshold(key)
    return _DERIVED[key]


def inference_planes(mask_logits, taxonomy, side, thresholds=THRESHOLDS):
    """One hand of one prompt, inference.py rule. mask_logits fp32 [H,W] on the device, taxonomy fp32 [4] on the device.
    Returns uint8 [len(thresholds), H, W] of 0/255 (all zero when the taxonomy gate closes this hand)."""
    ths = [sigmoid_logit_threshold(t) for t in thresholds]
    tax = None if taxonomy is None else taxonomy.reshape(-1)[:4].float().contiguous()   # None: the caller gated already
    return ops.gate_threshold_masks(mask_logits.contiguous(), ths, 255, tax, 1 if side == "left" else 0)


def chat_plane(mask_logits, taxonomy, side, on_value=100):
    """One hand of one prompt, chat.py rule: (mask > 0) * 100, zeros when the gate closes. Returns uint8 [H,W].
    The gate is the reference's: torch.argmax over the WHOLE per-frame taxonomy tensor [n_prompts, 4] flattened
    (chat.py:231,243) — index 1 blanks the left hand, index 0 the right one, any other index (>= 4 can only happen with more
    than one [SEG] in the answer) blanks neither. One host read of an index per frame; chat is interactive, not the hot path."""
    k = int(torch.argmax(taxonomy.reshape(-1)))
    if k == (1 if side == "left" else 0):
        return torch.zeros(mask_logits.shape[-2:], dtype=torch.uint8, device=mask_logits.device)
    return ops.gate_threshold_masks(mask_logits.contiguous(), [0.0], on_value, None, 1 if side == "left" else 0)[0]


# ---- robot_demo.py (2Haff/robot_demo.py:57-73,266-327): the heat map and the padded, ANDed mask of each written hand ----

def _octave_jet(x):
    """GNU Octave's jet.m at x in [0, 1] (exact fractions): what OpenCV's COLORMAP_JET tabulates (colormap.cpp, class Jet)."""
    from fractions import Fraction as F
    r = 4 * x - F(3, 2) if F(3, 8) <= x < F(5, 8) else (1 if F(5, 8) <= x < F(7, 8) else (F(9, 2) - 4 * x if x >= F(7, 8) else 0))
    g = 4 * x - F(1, 2) if F(1, 8) <= x < F(3, 8) else (1 if F(3, 8) <= x < F(5, 8) else (F(7, 2) - 4 * x if F(5, 8) <= x < F(7, 8) else 0))
    b = 4 * x + F(1, 2) if x < F(1, 8) else (1 if x < F(3, 8) else (F(5, 2) - 4 * x if x < F(5, 8) else 0))
    return r, g, b


def jet_table():
    """cv2.COLORMAP_JET as uint8 [256, 3] in RGB order (what cv2.imwrite of applyColorMap's BGR result holds on disk): Octave's jet
    sampled at i/255, times 255, rounded half to even (convertTo's cvRound). Restated: cv2 is not installed, so the table is not
    pinned against OpenCV's own float constants."""
    import numpy as np
    from fractions import Fraction
    return np.array([[round(255 * c) for c in _octave_jet(Fraction(i, 255))] for i in range(256)], dtype=np.uint8)


_JET_DEVICE = {}


def robot_planes(logits, th, margins, and_masks, on_value=255):
    """The outputs of one robot_demo.py request for the hands it writes, on the device (haff_robot_heatmap, haff_robot_mask).
    logits fp32 [n, H0, W0]: pred_masks_<hand>[i][0] of each written hand. th: --th, a LOGIT threshold. margins: (left, top, right,
    bottom). and_masks: n uint8 device tensors [H0 + top + bottom, W0 + left + right], the mask each hand is ANDed with.
    Returns (heat uint8 [n, H0, W0, 3] RGB = aff_<hand>_heat.png, masks uint8 [n, H1, W1] of 0 / on_value = aff_<hand>.png)."""
    import math
    logits = logits.float().contiguous()
    key = str(logits.device)
    if key not in _JET_DEVICE:
        _JET_DEVICE[key] = torch.from_numpy(jet_table()).to(logits.device)
    heat = ops.robot_heatmap(logits, _JET_DEVICE[key])
    # `pred_mask[pred_mask > th] = 1; pred_mask[pred_mask <= th] = 0` runs in place (:277-278): for th >= 1 the second line also
    # clears the ones the first one wrote, so no pixel survives
    t = float(th) if th < 1 else math.inf
    n, H0, W0 = logits.shape
    left, top, right, bottom = margins
    Ho, Wo = max(H0 + top + bottom, 0), max(W0 + left + right, 0)
    buf = torch.empty((n, (Ho * Wo + 3) // 4 * 4), dtype=torch.uint8, device=logits.device)   # 4-B aligned planes
    for k in range(n):
        ops.robot_mask(logits[k], t, margins, and_masks[k], on_value, out=buf[k, :Ho * Wo].view(Ho, Wo))
    return heat, buf[:, :Ho * Wo].view(n, Ho, Wo)


# ---- ActAffordance/scripts/utils/gaussian.py: the benchmark workflow's mask smoothing, on the logits (csrc/mask_smooth.hip) ----

def smooth_need(threshold=0.5):
    """The weight (of 65536) a pixel's "on" taps must reach for gaussian.py --threshold `threshold` to keep it on. The 8-bit blur of
    a 0/255 plane is (255 M + 32768) >> 16 with M the weight of the on taps, and `blurred / 255.0 > threshold` (in double, as numpy
    divides) holds from b = min{b in 0..255 : b / 255.0 > threshold} on: need = ceil((65536 b - 32768) / 255). 0.5 -> 32768."""
    t = float(threshold)
    if not 0.0 <= t < 1.0:       # NaN fails both
        raise ValueError(f"smoothing threshold {threshold}: must lie in [0, 1)")
    b = next(b for b in range(256) if b / 255.0 > t)
    return -((32768 - 65536 * b) // 255)


def smooth_mask_lists(masks_left, masks_right, threshold=0.5):
    """The two mask lists evaluate() returns (per frame fp32 [k, H0, W0] logits, k possibly 0) -> the same structure with every plane
    smoothed as gaussian.py smooths the PNGs written from it: `smoothed > x*(th)` is the 7x7 blur + threshold of `mask > x*(th)` for
    every th at once (ops.mask_quantile7). Both hands of a frame go through one launch; empty entries pass through."""
    need = smooth_need(threshold)
    out_left, out_right = list(masks_left), list(masks_right)
    for b, (ml, mr) in enumerate(zip(masks_left, masks_right)):
        if ml.shape[0] + mr.shape[0] == 0:
            continue
        # both hands of a frame have the frame's size; torch.cat of one non-empty and one empty entry is the non-empty one
        smoothed = ops.mask_quantile7(torch.cat([ml, mr]).float().contiguous(), need)
        if ml.shape[0]:
            out_left[b] = smoothed[:ml.shape[0]]
        if mr.shape[0]:
            out_right[b] = smoothed[ml.shape[0]:]
    return out_left, out_right
