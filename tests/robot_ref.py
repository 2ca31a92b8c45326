"""An independent CPU restatement of step 4 of the reference's robot loop (2Haff/robot_demo.py:57-73,266-327), written from the rules
of OpenCV 4.8 and Pillow with numpy and PIL only — it shares no code with the package.

  heatmap(x)          : create_heatmap. cv2.normalize(NORM_MINMAX, 0, 255) on float32 (scale = 255/(max-min) and shift = -min*scale
                        in double, scale 0 when max-min <= DBL_EPSILON; one fused multiply-add per value in float32), np.uint8
                        (truncation), applyColorMap(COLORMAP_JET) in the RGB order cv2.imwrite puts on disk, GaussianBlur((5, 5), 1)
                        on the 8-bit bit-exact path (fixed-point separable kernel, BORDER_REFLECT_101), integers only.
  pad_and_mask(x, ...): `x > th` -> 1, `x <= th` -> 0 in place, Image.fromarray (mode F) pasted into Image.new("L", padded size)
                        at (left, top), numpy & with the hand's mask (the other hand's when its own is missing), times 255 in uint8.
"""
import math
import sys

import numpy as np
from PIL import Image


def _half_even(v2):
    """round(v2 / 2), ties to even, for an integer v2"""
    q, r = divmod(v2, 2)
    return q + (r & q & 1)


def jet_table():
    """COLORMAP_JET (Octave's jet at i/255, x 255, ties to even) in RGB, from twice the channel value: piecewise linear in i with
    slope 8 and breakpoints at i = 32, 96, 160, 224 (x = 1/8, 3/8, 5/8, 7/8)."""
    t = np.zeros((256, 3), np.uint8)
    for i in range(256):
        r2 = 0 if i < 96 else (8 * i - 765 if i < 160 else (510 if i < 224 else 2295 - 8 * i))
        g2 = 0 if (i < 32 or i >= 224) else (8 * i - 255 if i < 96 else (510 if i < 160 else 1785 - 8 * i))
        b2 = 8 * i + 255 if i < 32 else (510 if i < 96 else (1275 - 8 * i if i < 160 else 0))
        t[i] = [_half_even(v) for v in (r2, g2, b2)]
    return t


def gaussian_coeffs(ksize=5, sigma=1.0, bits=8):
    """getGaussianKernelBitExact + getGaussianKernelFixedPoint_ED: exp(-d^2 / (2 sigma^2)) normalised to sum 1, then rounded from
    the outside in with the rounding error carried to the next tap; the centre takes what is left of 2^bits."""
    n2 = ksize // 2
    vals = [math.exp(-(d * d) / (2.0 * sigma * sigma)) for d in range(n2, 0, -1)]
    total = 1.0 + 2.0 * sum(vals)
    out, err, acc = [0] * ksize, 0.0, 0
    for i, v in enumerate(vals):
        adj = v / total * (1 << bits) + err
        v0 = int(round(adj))
        err = adj - v0
        out[i] = out[ksize - 1 - i] = v0
        acc += v0
    out[n2] = (1 << bits) - 2 * acc
    return tuple(out)


def fma32(x, a, b):
    """float32 fmaf(x, a, b), elementwise: x * a is exact in double; the double sum can round once more, which only matters when it
    lands exactly on a float32 midpoint — TwoSum gives the exact remainder that decides those."""
    p = np.asarray(x, np.float32).astype(np.float64) * np.float64(np.float32(a))
    bb = np.float64(np.float32(b))
    s = p + bb
    z = s - p
    err = (p - (s - z)) + (bb - z)
    r = s.astype(np.float32)
    lo = np.where(r.astype(np.float64) <= s, r, np.nextafter(r, np.float32(-np.inf)))
    hi = np.nextafter(lo, np.float32(np.inf))
    tie = (s == (lo.astype(np.float64) + hi.astype(np.float64)) / 2) & (err != 0)
    return np.where(tie, np.where(err > 0, hi, lo), r).astype(np.float32)


def normalize_u8(x):
    """np.uint8(cv2.normalize(x, None, 0, 255, cv2.NORM_MINMAX)) for a float32 plane"""
    x = np.asarray(x, np.float32)
    mn, mx = float(x.min()), float(x.max())
    d = mx - mn
    scale = 255.0 / d if d > sys.float_info.epsilon else 0.0
    shift = -mn * scale
    v = fma32(x, np.float32(scale), np.float32(shift))
    return np.clip(np.trunc(v), 0, 255).astype(np.uint8)


def reflect101(p, n):
    """borderInterpolate(p, n, BORDER_REFLECT_101) for an index array"""
    p = np.array(p)
    if n == 1:
        return np.zeros_like(p)
    while ((p < 0) | (p >= n)).any():
        p = np.where(p < 0, -p, np.where(p >= n, 2 * n - 2 - p, p))
    return p


def blur5(img):
    """GaussianBlur(img, (5, 5), 1) of a uint8 [H, W, C] image: sum c[dy] c[dx] p, + 2^15, >> 16"""
    c = gaussian_coeffs()
    H, W = img.shape[:2]
    a = img.astype(np.int64)
    h = sum(c[k] * a[:, reflect101(np.arange(W) + k - 2, W)] for k in range(5))
    v = sum(c[k] * h[reflect101(np.arange(H) + k - 2, H)] for k in range(5))
    return ((v + 32768) >> 16).astype(np.uint8)


_JET = jet_table()


def heatmap(x):
    """create_heatmap(x) as it lands on disk: uint8 [H, W, 3] RGB"""
    return blur5(_JET[normalize_u8(x)])


def pad_and_mask(x, th, margins, own, other=None):
    """aff_<hand>.png of one hand: margins = (left, top, right, bottom); own / other = the uint8 masks of this hand and of the other
    one (None when missing)"""
    left, top, right, bottom = margins
    pred = np.array(x, dtype=np.float32)
    pred[pred > th] = 1
    pred[pred <= th] = 0
    img = Image.fromarray(pred)
    w, h = img.size
    padded = Image.new("L", (w + left + right, h + top + bottom), color=0)
    padded.paste(img, (left, top))
    arr = np.array(padded)
    m = own if own is not None else other
    if m.shape != arr.shape:
        raise ValueError("cv2.bitwise_and: the sizes differ")
    return ((arr & m) * 255).astype(np.uint8)
