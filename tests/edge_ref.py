"""Plain CPU restatements, in float64, of the byte-moving kernels of csrc/elementwise.hip and the mask tail of
csrc/sam_decoder.hip, with the inputs that put those kernels at their edges and the tolerances the comparisons use.

Every function is written from the operation's definition (F.unfold, F.conv_transpose2d, F.interpolate, torch.argmax,
indexing, comparison) with torch on the CPU and numpy only. Nothing here imports the package or touches a GPU, so
tests/test_edge_ref_cpu.py can check the references and the tolerances on a machine without one.
"""
import numpy as np
import torch
import torch.nn.functional as F

U32 = 2.0 ** -24          # unit roundoff of fp32 (half an ulp of 1.0)
NAN, INF = float("nan"), float("inf")


def rand(shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return torch.randn(shape, generator=g) * scale


# ---------------------------------------------------------------------------------------------------------------- argmax
ARGMAX_V = (1, 5, 1023, 1024, 1025, 8191, 8192, 8193, 32003)


def argmax_rows(V, seed=0):
    """fp32 rows of width V at the argmax kernel's edges, as a [R, V] view of a wider tensor whose other columns hold +inf
    (a read past V wins visibly), and the name of each row. The kernel runs 1024 threads (16 waves of 64), thread t loads
    t, t + 1024, ... t + 7 * 1024 per trip and a trip covers 8192 entries; rows whose indices do not fit V are left out.
    Ties are pairs of 50.0 above N(0, 1) noise."""
    rows, names = [], []

    def add(name, r):
        names.append(name)
        rows.append(r)

    def noise(k):
        return rand((V,), seed * 100 + k)

    def tie(name, k, idx):
        if max(idx) < V:
            r = noise(k)
            r[list(idx)] = 50.0
            add(name, r)

    add("noise", noise(0))
    tie("tie in one thread's eight loads", 1, (3, 3 + 1024))
    tie("tie across waves", 2, (70, 5))
    tie("tie across waves, lower index in the later wave", 3, (70, 5 + 1024))
    tie("tie across trips", 4, (min(9, V - 8193), min(9, V - 8193) + 8192) if V > 8192 else (V,))
    tie("tie of the last entry", 5, (V // 2, V - 1))
    add("all equal", torch.full((V,), -3.25))
    add("all -inf", torch.full((V,), -INF))
    r = noise(6)
    r[V - 1] = 60.0
    add("maximum at V - 1", r)
    r = noise(7)
    r[0] = 50.0
    r[V // 2] = NAN
    add("one NaN", r)
    r = noise(8)
    r[V // 3] = INF
    r[2 * V // 3] = NAN
    add("one NaN after +inf", r)
    r = noise(9)
    r[V - 1] = NAN
    r[V // 2] = NAN
    add("two NaNs", r)
    tie_nan = noise(10)
    if V > 70 + 8192:
        tie_nan[[70 + 8192, 5 + 1024]] = NAN
        add("two NaNs across waves and trips", tie_nan)
    add("all NaN", torch.full((V,), NAN))
    return widen(torch.stack(rows), 13, INF)[:, :V], names


def widen(x, pad, fill):
    """x [R, C] copied into the left columns of a new [R, C + pad] tensor of `fill`: its [:, :C] view has a row stride > C"""
    wide = torch.full((x.shape[0], x.shape[1] + pad), fill, dtype=x.dtype)
    wide[:, :x.shape[1]] = x
    return wide


def argmax(x):
    return torch.argmax(x.detach().cpu(), dim=-1)


# ---------------------------------------------------------------------------------------------------------- upscale_mask
def upscale_inputs(n, h, w, seed):
    """fp32 CPU (up1 [n*h*w, 4*64], ln_w, ln_b, w2 [64, 4*32], b2, hyper [n, 32])"""
    return (rand((n * h * w, 256), seed), 1.0 + 0.2 * rand((64,), seed + 1), 0.3 * rand((64,), seed + 2),
            0.15 * rand((64, 128), seed + 3), 0.2 * rand((32,), seed + 4), rand((n, 32), seed + 5))


def upscale_mask(up1, ln_w, ln_b, w2, b2, hyper, n, h, w, eps=1e-6):
    """LayerNorm2d(64) -> GELU -> ConvTranspose2d(64 -> 32, k2, s2) -> GELU -> dot with hyper, in float64. up1 [n*h*w, 4*64] is the
    first transposed conv's output with columns (dy, dx, co); w2 [64, (dy2, dx2, c2)]. -> [n, 4h, 4w]"""
    up1, ln_w, ln_b, w2, b2, hyper = (t.detach().cpu().double() for t in (up1, ln_w, ln_b, w2, b2, hyper))
    u = up1.view(n, h, w, 2, 2, 64).permute(0, 5, 1, 3, 2, 4).reshape(n, 64, 2 * h, 2 * w)     # NCHW after the first ConvT
    mu = u.mean(1, keepdim=True)
    var = (u - mu).pow(2).mean(1, keepdim=True)
    u = (u - mu) / torch.sqrt(var + eps) * ln_w[None, :, None, None] + ln_b[None, :, None, None]
    u = 0.5 * u * (1.0 + torch.erf(u / np.sqrt(2.0)))
    weight = w2.view(64, 2, 2, 32).permute(0, 3, 1, 2).contiguous()                           # [in, out, kh, kw]
    u = F.conv_transpose2d(u, weight, b2, stride=2)
    u = 0.5 * u * (1.0 + torch.erf(u / np.sqrt(2.0)))
    return torch.einsum("nc,nchw->nhw", hyper, u)


# ------------------------------------------------------------------------------------------------------- resize_bilinear
# (planes, source HxW, crop HxW, output HxW)
RESIZE_CASES = (
    (2, (7, 9), (7, 9), (1, 1)),
    (2, (1, 1), (1, 1), (5, 6)),
    (2, (1, 40), (1, 33), (3, 77)),
    (3, (56, 56), (56, 56), (224, 224)),
    (2, (224, 224), (224, 168), (97, 131)),
    (2, (64, 48), (33, 20), (101, 77)),
)
RESIZE_BIG = (5, (256, 256), (256, 256), (1024, 1024))     # 5.24 M outputs: past the 16384 x 256 threads of one sweep


def resize_source(case, seed, outside=NAN):
    """fp32 [N, Hs, Ws] of N(0, 1); whatever lies outside the crop holds `outside` (NaN: a read there shows in the output)."""
    n, (hs, ws), (hc, wc), _ = case
    x = rand((n, hs, ws), seed)
    if outside is not None:
        fill = torch.full_like(x, outside) if isinstance(outside, float) else outside
        keep = torch.zeros((hs, ws), dtype=torch.bool)
        keep[:hc, :wc] = True
        x = torch.where(keep, x, fill)
    return x


def resize_bilinear(x, crop_hw, out_hw):
    """F.interpolate(bilinear, align_corners=False) of the float64 crop"""
    c = x.detach().cpu().double()[:, None, :crop_hw[0], :crop_hw[1]]
    return F.interpolate(c, tuple(out_hw), mode="bilinear", align_corners=False)[:, 0]


def resize_tol(l_max, adj_max, x_max):
    """Absolute bound on |fp32 bilinear - float64 bilinear| for one output, from (max(Hc, Wc), the largest difference between
    adjacent source samples along either axis, max |x|) of the crop.

    The source coordinate is f = s * (o + 0.5) - 0.5 with s = Hc / Ho. In fp32 the quotient, the product and the difference are
    each rounded once (o + 0.5 is exact), every intermediate is at most l_max in magnitude, so |df| <= 3 * U32 * l_max per axis
    (the clamp at 0 and the split into integer and fraction are exact). The interpolant is continuous and piecewise linear along
    each axis with slope at most adj_max per unit of coordinate, also across a cell boundary, so the two coordinate errors move
    the value by at most 2 * adj_max * |df|. The blend itself is a convex combination of four samples: 1 - l is rounded once and
    each sample passes through two products and at most two sums, all rounded (or fused), and the float64 value is rounded to
    fp32 once for the comparison: at most 8 roundings along any path, 8 * U32 * x_max. Higher-order terms are far below either."""
    return 2.0 * adj_max * 3.0 * U32 * l_max + 8.0 * U32 * x_max


def resize_case_tol(x, crop_hw):
    c = x.detach().cpu().double()[:, :crop_hw[0], :crop_hw[1]]
    adj = 0.0
    if c.shape[1] > 1:
        adj = max(adj, (c[:, 1:] - c[:, :-1]).abs().max().item())
    if c.shape[2] > 1:
        adj = max(adj, (c[:, :, 1:] - c[:, :, :-1]).abs().max().item())
    return resize_tol(max(crop_hw), adj, c.abs().max().item())


def resize_fp32(x, crop_hw, out_hw, half_pixel=True, clamp_to_crop=True):
    """The align_corners=False formula in numpy fp32, every operation rounded to fp32 as a GPU kernel's would be:
        f = max(scale * (o + 0.5) - 0.5, 0), i0 = min(int(f), crop - 1), i1 = min(i0 + 1, crop - 1), l = f - i0,
        out = (1 - ly) * ((1 - lx) * a + lx * b) + ly * ((1 - lx) * c + lx * d).
    half_pixel=False drops the + 0.5; clamp_to_crop=False lets i1 run to the source's edge instead of the crop's: the two
    mistakes the tolerance has to catch."""
    x = np.asarray(x.detach().cpu().numpy(), np.float32)
    f32 = np.float32

    def axis(crop, out, src):
        s = f32(crop) / f32(out)
        o = np.arange(out, dtype=np.float32) + (f32(0.5) if half_pixel else f32(0.0))
        f = np.maximum(s * o - f32(0.5), f32(0.0)).astype(np.float32)
        i0 = np.minimum(f.astype(np.int64), crop - 1)
        i1 = np.minimum(i0 + 1, (crop if clamp_to_crop else src) - 1)
        return i0, i1, (f - i0.astype(np.float32)).astype(np.float32)

    y0, y1, ly = axis(crop_hw[0], out_hw[0], x.shape[1])
    x0, x1, lx = axis(crop_hw[1], out_hw[1], x.shape[2])
    ly, lx = ly[None, :, None], lx[None, None, :]
    hy, hx = f32(1.0) - ly, f32(1.0) - lx
    a, b = x[:, y0][:, :, x0], x[:, y0][:, :, x1]
    c, d = x[:, y1][:, :, x0], x[:, y1][:, :, x1]
    return torch.from_numpy((hy * (hx * a + lx * b) + ly * (hx * c + lx * d)).astype(np.float32))


def max_err(got, ref):
    """max |got - ref| in float64; inf when got holds a non-finite value where ref is finite"""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    if not bool(torch.isfinite(got).all()):
        return INF
    return (got - ref).abs().max().item()


# ------------------------------------------------------------------------------------------------------------ thresholds
THRESHOLD_TOTALS = (1, 2, 3, 4, 5, 7, 1023, 4099)


def threshold_values(total, ths, seed):
    """fp32 [total]: N(0, 1) around the thresholds, with each threshold, its two fp32 neighbours, +-0, denormals, +-inf and NaN
    dealt over the positions in turn (so that short vectors get them too, a different one per seed)."""
    special = [0.0, -0.0, 1e-45, -1e-45, 1e-39, -1e-39, INF, -INF, NAN]
    for th in ths:
        t = np.float32(th)
        special += [float(t), float(np.nextafter(t, np.float32(INF))), float(np.nextafter(t, np.float32(-INF)))]
    sp = torch.tensor(special, dtype=torch.float32)
    x = rand((total,), seed) + next((float(t) for t in ths if np.isfinite(t)), 0.0)
    idx = torch.arange(total)
    put = (idx % 3 != 1) if total > len(special) else torch.ones(total, dtype=torch.bool)
    x[put] = sp[(idx[put] + seed) % len(special)]
    return x


def threshold(x, ths, on):
    """uint8 [len(ths), ...]: (x > th) * on, exactly"""
    x = x.detach().cpu()
    return torch.stack([(x > float(np.float32(th))).to(torch.uint8) * on for th in ths])


# ---------------------------------------------------------------------------------------------------------- softmax_rows
def softmax_rows_input(rows, C, seed):
    """fp32 [rows, C] of N(0, 1) whose first rows are the edges: +-80 and 1e4 (exp overflows without the max subtraction), equal
    values, -inf entries, one +inf. Row r takes edge r % 6 while r < 12, so a second block gets them too when rows > 64."""
    x = rand((rows, C), seed)
    for r in range(min(rows, 12)):
        k = r % 6
        if k == 0:
            x[r] = 80.0
            x[r, C // 2] = -80.0
        elif k == 1:
            x[r] *= 100.0
            x[r, 0] = 1e4
        elif k == 2:
            x[r] = -1e4
        elif k == 3:
            x[r, ::2] = -INF
            x[r, C - 1] = 2.5          # at least one finite entry
        elif k == 4:
            x[r, C - 1] = INF
    return x


def softmax_rows(x):
    """float64 softmax by its definition, exp(x - max) / sum. A row with one +inf has max = +inf, so its own entry is
    exp(inf - inf) = exp(NaN): the definition gives NaN for the whole row (torch.softmax agrees), and that is what is pinned."""
    x = x.detach().cpu().double()
    e = torch.exp(x - x.max(-1, keepdim=True).values)
    return e / e.sum(-1, keepdim=True)


# --------------------------------------------------------------------------------------------------------------- gathers
def patchify_nchw(x, P, gh, gw, Kp, out_dtype):
    """conv(k = s = P) rows by F.unfold of the top-left gh*P x gw*P of x [B, C, H, W]: [B*gh*gw, Kp], column (c, ky, kx), zero from
    C*P*P on; the (exact) values converted once to out_dtype"""
    x = x.detach().cpu().double()[:, :, :gh * P, :gw * P]
    rows = F.unfold(x, P, stride=P).transpose(1, 2).reshape(x.shape[0] * gh * gw, -1)
    return F.pad(rows, (0, Kp - rows.shape[1])).float().to(out_dtype)


SAM_MEAN, SAM_STD = (123.675, 116.28, 103.53), (58.395, 57.12, 57.375)


def patchify_u8(frames, P, gh, gw, Kp, mean3, std3):
    """float64 [B*gh*gw, Kp]: (u8 - mean) / std of the NHWC frame, zero where the gh*P x gw*P canvas has no frame (and from 3*P*P
    on), cut to the canvas, as conv rows. mean / std are the fp32 constants the entry point is handed."""
    fr = frames.detach().cpu().double().permute(0, 3, 1, 2)
    m = torch.tensor(np.asarray(mean3, np.float32).astype(np.float64)).view(1, 3, 1, 1)
    s = torch.tensor(np.asarray(std3, np.float32).astype(np.float64)).view(1, 3, 1, 1)
    xn = (fr - m) / s
    B, _, Hf, Wf = xn.shape
    canvas = torch.zeros((B, 3, gh * P, gw * P), dtype=torch.float64)
    hh, ww = min(Hf, gh * P), min(Wf, gw * P)
    canvas[:, :, :hh, :ww] = xn[:, :, :hh, :ww]
    rows = F.unfold(canvas, P, stride=P).transpose(1, 2).reshape(B * gh * gw, -1)
    return F.pad(rows, (0, Kp - rows.shape[1]))


def ulp32(ref):
    """spacing of fp32 at |ref| (float64 tensor)"""
    return torch.from_numpy(np.spacing(np.abs(ref.numpy()).astype(np.float32)).astype(np.float64))


def im2col3x3(x, via=torch.float64):
    """x [B, H, W, C] channels-last -> [B*H*W, 9*C] with column (ky, kx, c): F.unfold(kernel 3, padding 1) re-ordered. A pure copy,
    so `via` (the type the unfold runs in) only has to hold the input exactly."""
    B, H, W, C = x.shape
    cols = F.unfold(x.detach().cpu().to(via).permute(0, 3, 1, 2), 3, padding=1)          # [B, (c, ky, kx), H*W]
    return cols.view(B, C, 9, H * W).permute(0, 3, 2, 1).reshape(B * H * W, 9 * C).to(x.dtype)


def embed_splice(ids, pos, emb, img):
    """rows of emb for the ids left and right of the sentinel at pos[b], img[b] in its place -> [B, L + n_img - 1, Hd]"""
    ids, pos, emb, img = (t.detach().cpu() for t in (ids, pos, emb, img))
    return torch.stack([torch.cat([emb[ids[b, :int(pos[b])]], img[b], emb[ids[b, int(pos[b]) + 1:]]], 0)
                        for b in range(ids.shape[0])])


def add_bcast(a, b, mod):
    """a[r] + b[r % mod]: the float64 sum (exact for these formats) rounded to fp32, then once to the storage type"""
    a, b = a.detach().cpu(), b.detach().cpu()
    idx = torch.arange(a.shape[0]) % mod
    return (a.double() + b.double()[idx]).float().to(a.dtype)


def rope_table(Tmax, d):
    """fp32 [Tmax, d] = cos(d/2) | sin(d/2), base 10000 (an input of the kernel: the reference reads the same fp32 values)"""
    inv = 1.0 / (10000.0 ** (torch.arange(0, d, 2).double() / d))
    ang = torch.arange(Tmax).double()[:, None] * inv[None, :]
    return torch.cat([ang.cos(), ang.sin()], 1).float().contiguous()


def rope_cache(qkv, cs, B, Tq, Hq, Hkv, d, pos_rows):
    """float64 rotate-half RoPE of the q and k heads of qkv [B*Tq, >= (Hq + 2 Hkv) d] at positions pos_rows[b] + t.
    -> q [B, Tq, Hq, d], k [B, Tq, Hkv, d] rotated, v [B, Tq, Hkv, d] as read."""
    x = qkv.detach().cpu().double()[:, :(Hq + 2 * Hkv) * d].reshape(B, Tq, Hq + 2 * Hkv, d)
    cs = cs.detach().cpu().double()
    pos = torch.as_tensor(pos_rows).long()[:, None] + torch.arange(Tq)[None, :]                     # [B, Tq]
    cos = torch.cat([cs[pos][..., :d // 2]] * 2, -1)[:, :, None]
    sin = torch.cat([cs[pos][..., d // 2:]] * 2, -1)[:, :, None]

    def rot(t):
        return torch.cat([-t[..., d // 2:], t[..., :d // 2]], -1)
    q, k, v = x[:, :, :Hq], x[:, :, Hq:Hq + Hkv], x[:, :, Hq + Hkv:]
    return q * cos + rot(q) * sin, k * cos + rot(k) * sin, v
