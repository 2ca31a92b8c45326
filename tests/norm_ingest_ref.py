"""Plain CPU restatements of the row-norm and row-statistics kernels of csrc/norm.hip and of the frame-ingest kernels of
csrc/frame_ingest.hip, with the shapes and rows that put those kernels at their edges and the bounds the comparisons use.

The norm side is torch on the CPU: every function takes `dt`; torch.float64 is the reference, torch.float32 is the same formula
with every operation rounded to fp32 and the row sums added in the order of the kernel that the dispatch rule selects
(`selected_kernel`). The bound is train_edge_ref.bound (4 x that evaluation's own error + 8 fp32 ulps of the row's scale + half
an ulp of the storage type) plus the conditioning terms derived at `cond_terms`. Keyword flags switch on one deliberate mistake
each; tests/test_norm_ingest_ref_cpu.py shows that every one of them misses the bound. The frame-ingest side is integer numpy,
compared with array_equal. Nothing here imports the package or touches a GPU.
"""
import os
import sys
from fractions import Fraction

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_edge_ref as R   # noqa: E402

U32, F32, F64, BF16, F16, NAN, INF, SENT = R.U32, R.F32, R.F64, R.BF16, R.F16, R.NAN, R.INF, R.SENT
f32 = R.f32
EPS_LN, EPS_RMS = 1e-5, 1e-6
DENORM_FLOOR = R.FLOOR_ULPS * 2.0 ** -149      # below 2^-126 an fp32 operation rounds by up to 2^-150 absolute, not by U32 relative

# dtype code -> (type of x, type of y); 2 = fp32 rows in, bf16 rows out
NORM_CODES = {0: (BF16, BF16), 1: (F32, F32), 2: (F32, BF16), 3: (F16, F16)}
STATS_CODES = {0: BF16, 1: F32, 3: F16}
CODE_IDS = {0: "bf16", 1: "f32", 2: "f32-bf16", 3: "f16"}

# ----------------------------------------------------------------------------------------------------------------- shapes
# C: a partly filled chunk of 512 (8, 56, 72, 504, 520), the NCH arms 1 2 3 4 8 10 16 of the wave-per-row kernel entered below
# their width (1280: the ViT-H width, the only one on the 3 arm; 2568: 5 chunks on the 8 arm, 4104: 9 on the 10 arm, 5128: 11 on
# the 16 arm), both sides of the workgroup kernel's [2048, 6144] and the last supported width.
# rows: 1, 3, 4, 5 around the 4 rows of a block; 256 | 257 switch the kernel.
NORM_C = (8, 56, 64, 72, 504, 512, 520, 1280, 2040, 2048, 2056, 2568, 4096, 4104, 5128, 6144, 6152, 8184, 8192)
NORM_ROWS = (1, 3, 4, 5, 256, 257)
NORM_CASES = ((1, 8), (3, 56), (4, 64), (5, 72), (3, 504), (4, 512), (5, 520), (5, 1280), (256, 2040), (256, 2048), (257, 2048),
              (3, 2056), (257, 2056), (5, 2568), (257, 2568), (1, 4096), (256, 4096), (257, 4096), (4, 4104), (257, 4104), (3, 5128),
              (257, 5128), (256, 6144), (257, 6144), (256, 6152), (5, 6152), (3, 8184), (1, 8192), (5, 8192))
C_MAX = 8192
VALUE_C = (72, 1280, 4096)


def selected_kernel(rows, C, mapped=False):
    """launch_norm's rule: "wg" (one workgroup per row) exactly when there is no gather map, rows <= 256 and 2048 <= C <= 6144,
    else "wave" (one wave per row). haff_row_stats has the wave kernel only."""
    return "wg" if (not mapped and rows <= 256 and 2048 <= C <= 6144) else "wave"


def nch_arm(C):
    """the instantiated chunk count the wave-per-row dispatch runs C on"""
    nch = -(-C // 512)
    return next(n for n in (1, 2, 3, 4, 8, 10, 16) if nch <= n)


def chain(C, kernel):
    """additions on the longest path from one element of the row to the row's sum: 8 per 16-byte load of the busiest lane, 6 levels
    of the wave's xor tree, 2 more for the four waves of the workgroup kernel"""
    return 8 * -(-C // 512) + 6 if kernel == "wave" else 8 * -(-C // 2048) + 6 + 2


def row_sum(v, kernel):
    """sum over the last axis in the kernel's order: thread t of 64 (256) adds the 8 values of its 16-byte load at column
    8 (t + 64 i) (8 (t + 256 i)) one after the other, chunk after chunk; then the wave's xor tree; the workgroup kernel then adds
    its four waves as (w0 + w1) + (w2 + w3). Columns past C add nothing."""
    T = 64 if kernel == "wave" else 256
    rows, C = v.shape
    n = -(-C // (8 * T))
    p = torch.nn.functional.pad(v, (0, n * 8 * T - C)).reshape(rows, n, T, 8)
    acc = torch.zeros((rows, T), dtype=v.dtype)
    for i in range(n):
        for j in range(8):
            acc = acc + p[:, i, :, j]
    if kernel == "wave":
        return R.wave_sum(acc)
    w = R.wave_sum(acc.reshape(rows, 4, 64))
    return (w[:, 0] + w[:, 1]) + (w[:, 2] + w[:, 3])


def _exact_sum(v, kernel):
    return v.sum(-1)


# ------------------------------------------------------------------------------------------------------------ restatements
def row_stats(x, rms, eps, dt=F64, kernel="wave", var_c_minus_1=False, round_c_to_64=False, drop_last_8=False, rms_centred=False,
              eps_outside=False):
    """(mean [rows], rstd [rows]) of x [rows, C]: LayerNorm's biased two-pass variance, or RMSNorm's {0, rsqrt(mean(x^2) + eps)}.
    eps is the fp32 value the kernel receives. The flags are the mistakes the bound has to catch."""
    x = x.to(dt)
    rows, C = x.shape
    add = _exact_sum if dt == F64 else row_sum
    if drop_last_8:
        x = x[:, :C - 8] if C > 8 else x * 0
    n = float(-(-C // 64) * 64) if round_c_to_64 else float(C)
    e = torch.tensor(f32(eps), dtype=dt)
    n = torch.tensor(n, dtype=dt)

    def rstd_of(ms):
        return 1.0 / (torch.sqrt(ms) + e) if eps_outside else 1.0 / torch.sqrt(ms + e)
    if rms and not rms_centred:
        return torch.zeros(rows, dtype=dt), rstd_of(add(x * x, kernel) / n)
    mean = add(x, kernel) / n
    d = x - mean[:, None]
    var = add(d * d, kernel) / (n - 1 if var_c_minus_1 else n)
    return (torch.zeros(rows, dtype=dt) if rms else mean), rstd_of(var)


def norm(x, w, b, rms, eps, dt=F64, kernel="wave", **wrong):
    """y = (x - mean) * rstd * w + b (LayerNorm) or x * rstd * w (RMSNorm), unrounded in dt"""
    mean, rstd = row_stats(x, rms, eps, dt, kernel, **wrong)
    x = x.to(dt)
    if wrong.get("drop_last_8"):
        x = x.clone()
        x[:, x.shape[1] - 8:] = 0
    if wrong.get("rms_centred"):
        mean = row_stats(x, False, eps, dt, kernel)[0]
    if rms and not wrong.get("rms_centred"):
        return x * rstd[:, None] * w.to(dt)
    y = (x - mean[:, None]) * rstd[:, None] * w.to(dt)
    return y if b is None else y + b.to(dt)


def gather(y, in_map):
    """out row i = y[in_map[i]], every bit zero where in_map[i] < 0"""
    out = y[in_map.clamp_min(0).long()].clone()
    out[in_map < 0] = 0.0
    return out


def cond_terms(x, w, rms, eps, kernel):
    """(on y [rows, C], on mean [rows], on rstd [rows]): what the order of the kernel's additions may cost on a badly conditioned
    row, in addition to train_edge_ref.bound. That rule measures the error of ONE fp32 evaluation, and an evaluation can be right
    by luck: the partial sums of a constant row of 3.0 are all exact, those of 0.1 are not, and y = (x - mean) * rstd * w turns
    the difference into rstd = eps^-1/2 times as much. Derivation, with u = 2^-24 and n = chain(C, kernel) additions between one
    element and the row's sum: every addition rounds its partial sum by at most u of it, a partial sum is at most sum|x| in size,
    and an element passes through at most n of them, so |fl(sum x) - sum x| <= n u sum|x| and
        |d mean| <= n u mean|x|                                   (LayerNorm; the rounding of mean itself is one more u |mean|)
        |d y|    <= |d mean| rstd |w| + |y - b| (|d rstd| / rstd)
    The sum of squares has positive terms only, so its relative error is at most n u (+ 2 u for the square and the division):
        |d rstd| / rstd <= (n + 2) u / 2 + (d mean * rstd)^2 / 2  (the centre moved by d mean adds d mean^2 to the variance)
    For RMSNorm there is no mean: only the rstd term remains, with |y| = |x| rstd |w|."""
    x, w = x.double(), w.double()
    C = x.shape[1]
    n = chain(C, kernel)
    mean, rstd = row_stats(x, rms, eps)
    dmean = torch.zeros_like(rstd) if rms else (n + 1) * U32 * x.abs().mean(-1)
    rel = 0.5 * (n + 2) * U32 + 0.5 * (dmean * rstd) ** 2
    centred = x if rms else x - mean[:, None]
    dy = (dmean * rstd)[:, None] * w.abs() + (centred * rstd[:, None] * w).abs() * rel[:, None]
    clean = lambda t: torch.nan_to_num(t, nan=0.0, posinf=0.0, neginf=0.0)   # noqa: E731  (a NaN / inf row is compared bit for bit)
    return clean(dy) + DENORM_FLOOR, clean(dmean) + DENORM_FLOOR, clean(rstd * rel) + DENORM_FLOOR


def expect_norm(x, w, b, rms, eps, out_dtype, kernel, **wrong):
    """(float64 reference y, elementwise bound); with a `wrong` flag the REFERENCE stays right and only the fp32 evaluation, which
    then stands for a kernel with that mistake, is returned as a third value"""
    ref = norm(x, w, b, rms, eps)
    ev = norm(x, w, b, rms, eps, F32, kernel)
    bnd = R.bound(ref, ev, out_dtype, rowwise=True) + cond_terms(x, w, rms, eps, kernel)[0]
    return (ref, bnd, norm(x, w, b, rms, eps, F32, kernel, **wrong)) if wrong else (ref, bnd)


def expect_stats(x, rms, eps, **wrong):
    """((mean ref, bound), (rstd ref, bound)); haff_row_stats always runs the wave-per-row kernel"""
    (m, r), (m32, r32) = row_stats(x, rms, eps), row_stats(x, rms, eps, F32, "wave")
    _, cm, cr = cond_terms(x, torch.ones(x.shape[1]), rms, eps, "wave")
    scale_m = x.double().abs().mean(-1)
    scale_m = torch.where(torch.isfinite(scale_m), scale_m, torch.zeros_like(scale_m))
    floor = R.FLOOR_ULPS * 2 * U32
    out = ((m, R.K * _fin_err(m32, m) + floor * scale_m + cm), (r, R.K * _fin_err(r32, r) + floor * _fin(r) + cr))
    return out + (row_stats(x, rms, eps, F32, "wave", **wrong),) if wrong else out


def _fin(t):
    return torch.where(torch.isfinite(t), t.abs(), torch.zeros_like(t))


def _fin_err(ev, ref):
    return _fin(torch.where(torch.isfinite(ref), ev.double() - ref, torch.zeros_like(ref)))


WRONG_NORM = ({"var_c_minus_1": True}, {"round_c_to_64": True}, {"drop_last_8": True}, {"rms_centred": True}, {"eps_outside": True})


# ------------------------------------------------------------------------------------------------------------------ inputs
def norm_weights(C, seed):
    """w, b fp32 [C]: w around 1 with a zero and a negative entry"""
    w, b = 1.0 + 0.3 * R.rand((C,), seed + 1), 0.3 * R.rand((C,), seed + 2)
    w[0] = 0.0
    w[C // 2] = -0.75
    return w, b


def norm_inputs(rows, C, seed, dtype):
    """x [rows, C] in dtype: N(0.3, 2) as the older tests have it, row 0 with a larger offset"""
    x = R.rand((rows, C), seed, 2.0) + 0.3
    x[0] += 3.0
    return x.to(dtype)


def value_rows(C, seed, dtype, rms):
    """(x [R, C] in dtype, names): the named rows, bad rows between ordinary ones.
      constant 3         every partial sum exact: variance exactly 0, rstd = eps^-1/2
      constant 0.1       not exact in binary: what cond_terms is for
      large mean         mean / std = 1000 in fp32; in bf16 / f16 256 + 2 k (bf16's spacing there), k ~ N(0, 1.3): ~100
      f16 +-60000        RMSNorm only: sum of squares 3.6e9 C holds in fp32 where f16 itself would overflow
      denormal           every entry below the type's smallest normal number
      zero               rstd = eps^-1/2, y = b
      one NaN, one +inf  the row is non-finite where the reference is, the rows around it are not touched by it"""
    names, rows = [], []

    def add(name, r):
        names.append(name)
        rows.append(r.to(dtype).float())

    def ordinary(k):
        return R.rand((C,), seed + k, 2.0) + 0.3
    add("ordinary", ordinary(0))
    add("constant 3", torch.full((C,), 3.0))
    add("constant 0.1", torch.full((C,), 0.1))
    if dtype == F32:
        add("large mean", 1000.0 + R.rand((C,), seed + 1))
    else:
        add("large mean", 256.0 + 2.0 * torch.round(R.rand((C,), seed + 1) * 1.3))
    if dtype == F16 and rms:
        r = torch.full((C,), 60000.0)
        r[1::2] = -60000.0
        r[::3] *= 0.5
        add("f16 +-60000", r)
    tiny = 2.0 ** -24 if dtype == F16 else 2.0 ** -133          # the smallest denormal of f16 / of bf16 (a multiple of fp32's)
    add("denormal", tiny * torch.round(R.rand((C,), seed + 2) * 3.0))
    add("zero", torch.zeros(C))
    add("ordinary before NaN", ordinary(3))
    r = ordinary(4)
    r[C // 3] = NAN
    add("one NaN", r)
    add("ordinary between", ordinary(5))
    r = ordinary(6)
    r[2 * C // 3] = INF
    add("one +inf", r)
    add("ordinary after +inf", ordinary(7))
    return torch.stack(rows).to(dtype), names


MAP_CASES = ("all -1", "duplicates", "longer than the input", "permutation")


def gather_map(name, rows_in):
    """int32 [rows_out]; rows_out is never a multiple of 4 except for the all -1 map of 4 rows"""
    if name == "all -1":
        return torch.full((4,), -1, dtype=torch.int32)
    if name == "duplicates":
        return torch.tensor([rows_in - 1, 0, 0, -1, rows_in - 1], dtype=torch.int32)
    if name == "longer than the input":
        m = torch.arange(2 * rows_in + 3, dtype=torch.int32) % rows_in
        m[1::4] = -1
        return m
    return torch.arange(rows_in - 1, -1, -1, dtype=torch.int32)


# ---------------------------------------------------------------------------------------------------------------- finalize
FINALIZE_ROWS = (1, 255, 256, 257)
FINALIZE_SLOTS = (1, 2, 20, 65)               # 20 slots of 64 = 1280, the width the producer GEMMs run at
FINALIZE_PATTERNS = ("ratio 100", "ratio 1000", "ordinary", "negative", "zero")
FINALIZE_EPS = 1e-6


def finalize_partials(rows, slots, seed=0):
    """fp32 [rows, slots, 2] = {sum, sum of squares} of 64 columns each, and the pattern name of every row. Whatever the values,
    the double sums of <= 65 fp32 numbers of one size are exact (24 + 7 bits < 53), so the partials ARE the data: nothing is lost
    before the arithmetic under test.
      ratio 100 / 1000   columns m +- 1 in turn with m = 100 (+ row % 7) | 1000 (+ row % 7): slot = {64 m, 64 (m^2 + 1)}, both exact
                         in fp32; the variance is exactly 1
      ordinary           the fp32-rounded slot sums of N(0.3, 2) columns
      negative           columns all m = fl32(1.1): slot = {64 m, the fp32 number below 64 m^2}: E[x^2] - mean^2 < 0, clamped to 0
      zero               all-zero sums: rstd = eps^-1/2"""
    part = np.zeros((rows, slots, 2), dtype=np.float32)
    names = []
    rng = np.random.default_rng(seed + 1000 * rows + slots)
    for r in range(rows):
        name = FINALIZE_PATTERNS[r % len(FINALIZE_PATTERNS)]
        names.append(name)
        if name.startswith("ratio"):
            m = float(name.split()[1]) + r % 7
            part[r, :, 0], part[r, :, 1] = 64 * m, 64 * (m * m + 1)
            assert float(part[r, 0, 1]) == 64 * (m * m + 1)
        elif name == "ordinary":
            x = rng.standard_normal((slots, 64)) * 2 + 0.3
            part[r, :, 0], part[r, :, 1] = x.sum(1), (x * x).sum(1)
        elif name == "negative":
            m = np.float32(1.1)
            part[r, :, 0] = np.float32(64) * m
            part[r, :, 1] = np.nextafter(np.float32(64.0 * float(m) * float(m)), np.float32(0))
    return part, names


def finalize_exact(part, C, eps):
    """(mean, rstd) float64 [rows] in exact rational arithmetic up to the square root, and |mean| / std per row (inf when the
    variance is clamped)"""
    rows, slots, _ = part.shape
    mean, rstd, ratio = np.zeros(rows), np.zeros(rows), np.zeros(rows)
    e = Fraction(f32(eps))
    for r in range(rows):
        s1 = sum((Fraction(float(v)) for v in part[r, :, 0]), Fraction(0))
        s2 = sum((Fraction(float(v)) for v in part[r, :, 1]), Fraction(0))
        m = s1 / C
        var = max(s2 / C - m * m, Fraction(0))
        mean[r], rstd[r] = float(m), 1.0 / np.sqrt(float(var + e))
        ratio[r] = abs(float(m)) / np.sqrt(float(var)) if var > 0 else INF
    return mean, rstd, ratio


def finalize(part, C, eps, inv_c_fp32=False):
    """the kernel's arithmetic: slots added in order in double, divided by C in double (inv_c_fp32: multiplied by the fp32 number
    nearest to 1 / C instead, the earlier form), difference clamped at 0, results rounded to fp32"""
    s = part.astype(np.float64).cumsum(1)[:, -1]
    if inv_c_fp32:
        ic = float(np.float32(1.0) / np.float32(C))
        mean, ex2 = s[:, 0] * ic, s[:, 1] * ic
    else:
        mean, ex2 = s[:, 0] / C, s[:, 1] / C
    var = np.maximum(ex2 - mean * mean, 0.0)
    return mean.astype(np.float32), (1.0 / np.sqrt(var + f32(eps))).astype(np.float32)


def finalize_bounds(mean, rstd, C, eps):
    """2 fp32 ulps on mean (its own rounding is half of one). rstd: 2 fp32 ulps plus what double arithmetic leaves of the
    cancellation in E[x^2] - mean^2: the two quotients and the product round by 2^-53 of E[x^2] ~ mean^2 each, so the variance
    carries at most 4 * 2^-53 * mean^2 and rstd half of that relative to var + eps: 2 * 2^-53 * mean^2 * rstd^2. With exact
    partials nothing of the order 2^-24 (mean / std)^2 is left: that term belongs to partials which were themselves rounded to
    fp32 by their producer, and is their producer's."""
    bm = 2 * 2 * U32 * np.abs(mean) + 2.0 ** -149
    br = rstd * (2 * 2 * U32 + 2 * 2.0 ** -53 * (mean * rstd) ** 2)
    return bm, br


# ------------------------------------------------------------------------------------------------------------ frame ingest
GRID_CAP = 65536 * 256          # threads of one sweep of the three kernels (grid_1d)
# (Hin, Win) -> (Hout, Wout): extents of 1 in and out, single-axis calls (one side already matches), 4000 taps, 2 -> 257
GEOMETRIES = (((1, 1), (5, 7)), ((1, 9), (4, 3)), ((9, 1), (3, 4)), ((7, 5), (1, 1)), ((2, 3), (3, 2)), ((3, 2), (2, 3)),
              ((4000, 3), (1, 3)), ((3, 4000), (3, 1)), ((2, 2), (257, 255)), ((6, 5), (6, 11)), ((6, 5), (13, 5)), ((9, 8), (9, 3)),
              ((9, 8), (4, 8)))
IMAGE_KINDS = ("random", "checkerboard", "all 0", "all 255")
FILTERS = ("bilinear", "bicubic")
# the smallest batches of 3 that pass the cap by a ragged amount: axis 0 counts output PIXELS (3 x 1366 x 4095 = cap + 4094),
# axis 1 output BYTES (3 x 5 x 372830 x 3 = cap + 134)
OVER_CAP = {0: (3, (1366, 5), (1366, 4095)), 1: (3, (2, 372830), (5, 372830))}


def image(kind, B, H, W, seed=0):
    """uint8 [B, H, W, 3]; the checkerboard has 0 / 255 cells of 2 x 2 pixels, shifted by one cell per channel and per frame:
    bicubic's negative taps overshoot at every step of it, and both clips run"""
    if kind == "random":
        return np.random.default_rng(seed).integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    if kind == "checkerboard":
        b, y, x, c = np.ogrid[0:B, 0:H, 0:W, 0:3]
        return (((b + y // 2 + x // 2 + c) % 2) * 255).astype(np.uint8)
    return np.full((B, H, W, 3), 0 if kind == "all 0" else 255, dtype=np.uint8)


def resample_axis(img, axis, bounds, coeffs):
    """One pass of Pillow's 8-bit resampling on uint8 [B, H, W, 3]: axis 0 resamples W, axis 1 resamples H.
    out = clip8((2^21 + sum_t in[first + t] * coeff[t]) >> 22); the int32 accumulator of the kernel must not overflow."""
    img = np.moveaxis(img, 2 if axis == 0 else 1, 0).astype(np.int64)
    out = np.empty((bounds.shape[0],) + img.shape[1:], dtype=np.uint8)
    for o in range(bounds.shape[0]):
        x0, n = int(bounds[o, 0]), int(bounds[o, 1])
        assert 0 <= x0 and x0 + n <= img.shape[0] and n <= coeffs.shape[1]
        acc = (1 << 21) + np.tensordot(coeffs[o, :n].astype(np.int64), img[x0:x0 + n], 1)
        assert np.abs(acc).max() < 2 ** 31, "the int32 accumulator overflows"
        out[o] = np.clip(acc >> 22, 0, 255)
    return np.ascontiguousarray(np.moveaxis(out, 0, 2 if axis == 0 else 1))


def resize(img, out_hw, filt, tables):
    """Image.resize((out_w, out_h), filt): horizontal pass, uint8 intermediate, vertical pass; a pass whose extent already matches
    is left out. tables(n_in, n_out, filt) -> (bounds, coeffs)"""
    H, W = img.shape[1:3]
    if out_hw[1] != W:
        img = resample_axis(img, 0, *tables(W, out_hw[1], filt))
    if out_hw[0] != H:
        img = resample_axis(img, 1, *tables(H, out_hw[0], filt))
    return img


def clip_normalize(img, top, left, S, lut):
    """float32 [B, 3, S, S] = lut[c][img[b, top + y, left + x, c]]"""
    crop = img[:, top:top + S, left:left + S, :]
    return np.stack([lut[c][crop[..., c]] for c in range(3)], 1).astype(np.float32)


def every_byte_frame(B, H, W):
    """uint8 [B, H, W, 3] holding every byte value in every channel (H * W >= 256), a different order per channel and frame"""
    assert H * W >= 256
    b, p, c = np.ogrid[0:B, 0:H * W, 0:3]
    return ((p * (2 * c + 1) + 37 * c + 101 * b) % 256).astype(np.uint8).reshape(B, H, W, 3)


# (B, (H, W), top, left, S): asymmetric offsets, S = 1, S equal to the frame, non-square frames
CLIP_CASES = ((2, (16, 16), 0, 0, 16), (1, (17, 23), 3, 5, 11), (3, (23, 17), 6, 0, 17), (2, (16, 19), 15, 18, 1),
              (1, (20, 31), 0, 11, 20))
CLIP_OVER_CAP = (3, (1367, 1368), 1, 2, 1366)      # 3 x 3 x 1366^2 = cap + 16388 outputs
