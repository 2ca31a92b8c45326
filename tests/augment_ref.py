"""CPU restatement of csrc/frame_augment.hip in integer / fp32 numpy, written from the arithmetic Pillow's C code performs
(ImagingBlend, rgb2l, ImageStat's mean) and not from the kernels, and the Pillow routes the tests compare against.

    L(r,g,b)       = (19595 r + 38470 g + 7471 b + 32768) >> 16
    blend(d, i, f) = clip8(trunc(fl32(fl32(d) + fl32(f * fl32(i - d)))))     product and sum round separately
    p1 = blend(0, p, fb);  S = sum L(p1), m = (2 S + n) div 2 n;  p2 = blend(m, p1, fc);  p3 = blend(L(p2), p2, fs)
"""
import numpy as np

# (f, d, i, what Pillow gives = the separately rounded form, what a fused multiply-add would give): found by search on the CPU
FMA_TRIPLES = [(0.5270936489105225, 236, 33, 129, 128), (1.0650407075881958, 132, 9, 1, 0), (0.6903225183486938, 22, 177, 129, 128),
               (1.038167953491211, 137, 6, 1, 0), (1.3174601793289185, 46, 109, 129, 128)]


def luma(rgb):
    """uint8 [..., 3] -> int64 [...]: Pillow's RGB -> L."""
    c = rgb.astype(np.int64)
    return (19595 * c[..., 0] + 38470 * c[..., 1] + 7471 * c[..., 2] + 32768) >> 16


def blend(d, i, f):
    """Image.blend(degenerate d, image i, f) per byte; d and i broadcast. Every step is one fp32 operation."""
    d, i = np.asarray(d, dtype=np.int64), np.asarray(i, dtype=np.int64)
    f = np.float32(f)
    prod = (f * (i - d).astype(np.float32)).astype(np.float32)
    t = (d.astype(np.float32) + prod).astype(np.float32)
    return np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.uint8)


def blend_fused(d, i, f):
    """The same with the product left unrounded (what a fused multiply-add computes): the form the kernels must NOT take."""
    t = (np.float64(d) + np.float64(np.float32(f)) * np.float64(i - d)).astype(np.float32)
    return int(0 if t <= 0 else 255 if t >= 255 else np.trunc(t))


def jitter_sum(frame, fb):
    """S of haff_jitter_stats_u8: the sum of L over the brightness-scaled frame."""
    return int(luma(blend(0, frame, fb)).sum())


def jitter_mean(frame, fb):
    n = frame.shape[0] * frame.shape[1]
    return (2 * jitter_sum(frame, fb) + n) // (2 * n)


def jitter(frame, factors):
    """uint8 [H,W,3] -> ImageEnhance.Brightness -> Contrast -> Color with (fb, fc, fs)."""
    fb, fc, fs = factors
    p1 = blend(0, frame, fb)
    p2 = blend(jitter_mean(frame, fb), p1, fc)
    return blend(luma(p2)[..., None], p2, fs)


def augment(frame, flip, factors):
    out = jitter(frame, factors) if factors is not None else frame
    return np.ascontiguousarray(out[:, ::-1]) if flip else out.copy()


# ---- Pillow itself ----------------------------------------------------------------------------------------------------------------
def pil_jitter(frame, factors):
    from PIL import Image, ImageEnhance
    im = Image.fromarray(frame, "RGB")
    for enhance, f in zip((ImageEnhance.Brightness, ImageEnhance.Contrast, ImageEnhance.Color), factors):
        im = enhance(im).enhance(f)
    return np.asarray(im)


def pil_flip(frame):
    from PIL import Image
    return np.asarray(Image.fromarray(frame).transpose(Image.FLIP_LEFT_RIGHT))


def pil_augment(frame, flip, factors):
    out = pil_jitter(frame, factors) if factors is not None else frame
    return np.ascontiguousarray(pil_flip(out) if flip else out)


def pil_blend_1x1(d, i, f):
    from PIL import Image
    return int(np.asarray(Image.blend(Image.new("L", (1, 1), d), Image.new("L", (1, 1), i), f))[0, 0])


# ---- shared cases -----------------------------------------------------------------------------------------------------------------
def fp32(x):
    return float(np.float32(x))


def random_frame(hw, seed, kind="plain"):
    x = np.random.default_rng(seed).integers(0, 256, tuple(hw) + (3,), dtype=np.uint8)
    if kind == "dark":
        return x // 8
    if kind == "bright":
        return (255 - x // 16).astype(np.uint8)
    return x


def tie_frame():
    """1 x 2 grey frame of L 10 and 11: mean 10.5, Pillow's int(mean + 0.5) = 11."""
    return np.array([[[10, 10, 10], [11, 11, 11]]], dtype=np.uint8)


def staged_frame(d, i, hw=(4, 8)):
    """A grey frame whose contrast-stage mean is exactly d and that holds a pixel with channel value i: with fb = 1 the contrast
    blend of that pixel is blend(d, i, fc) on real data. n - 1 pixels share the remainder of the sum n d - i as evenly as bytes allow."""
    n = hw[0] * hw[1]
    rest = n * d - i
    assert 0 <= rest <= 255 * (n - 1)
    vals = np.full(n - 1, rest // (n - 1), dtype=np.int64)
    vals[:rest % (n - 1)] += 1
    grey = np.concatenate([[i], vals]).astype(np.uint8).reshape(hw)
    frame = np.repeat(grey[..., None], 3, -1)
    assert jitter_mean(frame, 1.0) == d and luma(frame)[0, 0] == i
    return frame
