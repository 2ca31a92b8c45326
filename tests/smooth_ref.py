"""An independent CPU restatement of step 2 of the reference's benchmark workflow (ActAffordance/scripts/utils/gaussian.py:
cv2.GaussianBlur(img, (7, 7), 0), `blurred / 255.0 > tau`, back to 0 / 255), and of the selection filter the package runs instead on
the fp32 logits. numpy only; it shares no code with the package.

  blur7(img)                : the 8-bit bit-exact blur. sigma = 0 at ksize 7 takes OpenCV's built-in table {0.03125, 0.109375, 0.21875,
                              0.28125, ...}, exactly {8, 28, 56, 72, 56, 28, 8} / 256; BORDER_REFLECT_101; integers only,
                              out = (sum c[dy] c[dx] p + 2^15) >> 16.
  files_route(logit, lt, tau): what the files hold after inference.py wrote `logit > lt` as 0 / 255 and gaussian.py --threshold tau
                              went over it.
  need(tau)                 : the weight of "on" taps (of 65536) from which files_route keeps a pixel on.
  quantile7(logit, need)    : per pixel the largest tap value v with weight{taps >= v} >= need; NaN taps count as -inf.

The identity the product rests on: 255 [quantile7(logit, need(tau)) > lt] == files_route(logit, lt, tau) for every lt.

The keyword arguments of quantile7 are the one-mistake-at-a-time variants tests/test_smooth_ref_cpu.py shows to fail; the defaults
are the rule.
"""
import numpy as np

COEFFS = (8, 28, 56, 72, 56, 28, 8)
TOTAL = 65536


def reflect101(p, n):
    """gfedcb|abcdefgh|gfedcba for an index array, any overshoot"""
    p = np.array(p)
    if n == 1:
        return np.zeros_like(p)
    while ((p < 0) | (p >= n)).any():
        p = np.where(p < 0, -p, np.where(p >= n, 2 * n - 2 - p, p))
    return p


def reflect(p, n):
    """BORDER_REFLECT (the wrong one): fedcba|abcdefgh|hgfedcb"""
    p = np.array(p)
    if n == 1:
        return np.zeros_like(p)
    while ((p < 0) | (p >= n)).any():
        p = np.where(p < 0, -p - 1, np.where(p >= n, 2 * n - 1 - p, p))
    return p


def blur7(img):
    """GaussianBlur(img, (7, 7), 0) of a 2-D uint8 image"""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 2
    H, W = img.shape
    a = img.astype(np.int64)
    h = sum(COEFFS[k] * a[:, reflect101(np.arange(W) + k - 3, W)] for k in range(7))
    v = sum(COEFFS[k] * h[reflect101(np.arange(H) + k - 3, H)] for k in range(7))
    return ((v + 32768) >> 16).astype(np.uint8)


def files_route(logit, lt, tau=0.5):
    plane = ((np.asarray(logit, np.float32) > np.float32(lt)).astype(np.uint8) * 255)
    return ((blur7(plane) / 255.0 > tau).astype(np.uint8) * 255)


def need(tau=0.5):
    """blurred = (255 M + 32768) >> 16 >= b  <=>  255 M >= 65536 b - 32768, for b the first level with b / 255.0 > tau"""
    b = min(b for b in range(256) if b / 255.0 > tau)
    num = 65536 * b - 32768
    return num // 255 + (1 if num % 255 else 0)


def taps(plane, border=reflect101):
    """[H, W, 49] taps of a 2-D array, index dy * 7 + dx"""
    H, W = plane.shape
    ys = [border(np.arange(H) + d - 3, H) for d in range(7)]
    xs = [border(np.arange(W) + d - 3, W) for d in range(7)]
    return np.stack([plane[ys[dy]][:, xs[dx]] for dy in range(7) for dx in range(7)], axis=-1)


def quantile7(logit, need_, *, border=reflect101, strict=False, cy=COEFFS, cx=COEFFS, nan_as=-np.inf):
    """float32 [H, W] -> float32 [H, W]. Variants: border=reflect, strict=True (`>` for `>=`), cy / cx (per-axis tables), nan_as=inf."""
    x = np.array(logit, dtype=np.float32)
    x = np.where(np.isnan(x), np.float32(nan_as), x).astype(np.float32)
    t = taps(x, border)
    w = np.array([cy[dy] * cx[dx] for dy in range(7) for dx in range(7)], dtype=np.int64)
    order = np.argsort(-t.astype(np.float64), axis=-1, kind="stable")          # descending; -inf last
    ts = np.take_along_axis(t, order, axis=-1)
    cum = np.cumsum(w[order], axis=-1)
    # the first position whose cumulated weight reaches need: every larger value has less weight at or above it
    reached = (cum > need_) if strict else (cum >= need_)
    first = np.argmax(reached, axis=-1)
    out = np.take_along_axis(ts, first[..., None], axis=-1)[..., 0]
    return np.where(reached.any(axis=-1), out, np.float32(-np.inf)).astype(np.float32)


def smoothed_plane(logit, lt, need_, **variant):
    """255 [quantile7 > lt] as uint8"""
    return ((quantile7(logit, need_, **variant) > np.float32(lt)).astype(np.uint8) * 255)


# ---- inputs shared by the CPU and the GPU tests ----

def fields(shape, rng):
    """(name, float32 plane): Gaussian, integer-rounded (ties everywhere), planted NaN / +-inf / +-0.0"""
    H, W = shape
    g = (rng.standard_normal(shape) * 3).astype(np.float32)
    yield "gaussian", g
    yield "integers", np.round(rng.standard_normal(shape) * 2).astype(np.float32)
    p = (rng.standard_normal(shape) * 3).astype(np.float32)
    kind = rng.integers(0, 12, shape)
    for k, v in ((0, np.nan), (1, np.inf), (2, -np.inf), (3, 0.0), (4, -0.0)):
        p[kind == k] = np.float32(v)
    yield "planted", p
    yield "mostly_nan", np.where(rng.random(shape) < 0.6, np.float32(np.nan), g).astype(np.float32)


def stripes(shape, lo=-4.0, hi=3.0):
    """two-valued planes with a 1- and a 2-pixel stripe, vertical at columns 63 | 64 and horizontal at rows 15 | 16 (a 64 x 16
    tile's seams) when the plane reaches them, else at the middle"""
    H, W = shape
    cx = 63 if W >= 65 else max(W // 2 - 1, 0)
    cy = 15 if H >= 17 else max(H // 2 - 1, 0)
    for width in (1, 2):
        v = np.full(shape, lo, np.float32)
        v[:, cx:cx + width] = hi
        yield f"v{width}", v, ("v", cx, width)
        h = np.full(shape, lo, np.float32)
        h[cy:cy + width, :] = hi
        yield f"h{width}", h, ("h", cy, width)


def index_planes(shape, rng):
    """every value distinct and naming its own position: a ramp, and a seeded permutation of it with mixed signs"""
    H, W = shape
    ramp = np.arange(H * W, dtype=np.float32).reshape(shape)
    yield "ramp", ramp
    perm = rng.permutation(H * W).astype(np.float32).reshape(shape) - np.float32(H * W // 2) + np.float32(0.5)
    yield "permutation", perm


LOGIT_THRESHOLDS = (-2.5, -1.0, 0.0, 2.0 ** -23.4, 1.0, 2.5)
