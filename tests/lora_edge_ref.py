"""Plain torch restatements of the rank-r adapter kernels of csrc/lora.hip that had no direct test (the q|k|v + RoPE forward with two
and three adapters, its adjoint, dx with no / one / two / three masks) and of haff_lora_tn, with the inputs that put those kernels
at their edges, the shape lists and the bounds the comparisons use. Built on tests/train_edge_ref.py (bound, ratio, half_ulp,
sum_bound_abs, K = 4, FLOOR_ULPS = 8, SENT).

Every restatement takes `dt`: torch.float64 is the reference; torch.float32 is the same formula with the kernels' documented
roundings and no others (16-bit operands, fp32 arithmetic; the one rounding to the 16-bit type at the store is the bound's half
storage ulp; dx with accumulate rounds old + update once). The functions run on the device their tensors are on: the past-the-cap
cases evaluate them in float64 on the GPU in row slabs (`row0`), torch's float64 elementwise operations and matmul not being the
code under test. Keyword flags switch on one deliberate mistake each (FWD_MISTAKES, BWD_MISTAKES, DX_MISTAKES, TN_MISTAKES, and the
buffer-level ones of `embed`); tests/test_lora_edge_ref_cpu.py shows that every one of them misses its criterion.

Two input families. Exact: small integers, masks in {0, 1, 2}, a power-of-two scale and RoPE tables of quarter turns, sized so that
every product, partial sum and result is an integer of magnitude <= 256: exact in fp32 in any order and storable in bf16 and f16,
so the comparison is ==. Gauss: the magnitudes of tests/test_lora_fullsize_gpu.py, held to
    bound = K * max |fp32 evaluation - float64| + FLOOR_ULPS fp32 ulps of the sum of absolute terms + half a storage ulp
(`bound(ref, ev32, dtype, scale=abs_sum)`). Nothing here imports the package or needs a GPU."""
import torch

from train_edge_ref import BF16, F16, F32, F64, FLOOR_ULPS, K, NAN, SENT, U32, bound, f32, half_ulp, ratio, rope_table, sum_bound_abs  # noqa: F401

HD = 128                  # head dim (lora.hip: HD)
HALF = (BF16, F16)
IDS = {BF16: "bf16", F16: "f16"}
EXACT_MAX = 256           # integers up to 2^8 are values of bf16 (8 significand bits) and of f16
OLD_TOL = 3e-2            # the widest max-norm tolerance of the node-level tests: max|err| <= OLD_TOL * max|ref|


def _up(n, m):
    return -(-n // m) * m


# ------------------------------------------------------------------------------------------------------------- shape lists
# M of the forward, the adjoint and dx. A workgroup is 4 waves x one 16-row tile each (`rt = blockIdx.y * 4 + wave`).
ROWS = (1,        # one row: 15 lanes of the only tile clamped to row 0 (`rc = valid ? row : p.M - 1`), waves 1-3 idle (`rt < n_rt`)
        15,       # the tile one row short: `if (valid) store8h`
        16,       # the tile exactly full
        17,       # a second tile of one row, on wave 1
        63,       # four tiles, the fourth one row short
        64,       # the workgroup exactly full: `gy = (n_rt + 3) / 4` = 1
        65,       # gridDim.y = 2, the second workgroup with one row (bwd: `i < total` cuts the third block at 65 * nh * 8 threads)
        100)      # seven tiles, the last of 4 rows; 7 does not divide 100
WIDTHS = (128, 384)       # H (forward / adjoint: `head = blockIdx.x`, 1 and 3 heads) and K (dx: `c0 = blockIdx.x * 128`)
LAYOUTS = ("tight", "padded", "odd")
TN_M = (1,        # one row block of one row: 15 rows of the only step masked (`m0 + i < r_hi`), waves 1-3 skip (`if (m0 < r_hi)`)
        15, 16,   # the first wave's step one row short / full
        17,       # wave 1 takes one row
        63, 64,   # the fourth wave's step one row short / the 64-row block full (`more` false for every wave)
        65,       # rows_per_block stays 64 (`rpb < 64 ? 64`): a second row block of one row
        1024,     # ceil(M / 16) = 64: 16 full blocks of 64
        1025,     # ceil(M / 16) = 65 -> rows_per_block 128, 9 blocks, the last of one row; `more` true once per wave
        1039)     # the last block of 15 rows
TN_N = (2,        # one column pair: lanes 1-63 compute on column 0 (`colc = col < N ? col : 0`) and drop it (`if (n < N)`)
        126,      # the last lane of the only column block past N
        128,      # the column block exactly full
        130)      # a second column block with one live lane
TN_R = (8, 16)


def t_values(M):
    """T: one position for every row, 7 (no divisor of most M: the position wraps inside a tile) and M (never wraps)"""
    return (1, 7, M)


def lds(layout, M, width):
    """leading dimensions of one case. tight: every ld its minimum (ldt = M: odd for odd M). padded: 8 more columns on every
    16-byte operand (ld_qkv = 3H + 8, ldo = ld_in = H + 8, ld_out = 3H + 8, ldk = ldx = K + 8), t^T on roundup(M, 16) as the
    trainer lays it out. odd: ldt = M + 5, lda = K + 3 (both are read with scalar loads and have no alignment rule)."""
    pad = 8 if layout == "padded" else 0
    return dict(w=width + pad, w3=3 * width + pad, ldt={"tight": M, "padded": _up(M, 16), "odd": M + 5}[layout],
                lda=width + (3 if layout == "odd" else 0))


def tn_geometry(M):
    """(rows_per_block, row blocks) as lora_tn_rows_per_block and lora_tn_ws of lora.hip state them: about 16 row blocks, each a
    multiple of 64 rows"""
    rpb = max(64, _up(-(-M // 16), 64))
    return rpb, -(-M // rpb)


assert [tn_geometry(M) for M in (1, 15, 16, 17, 63, 64)] == [(64, 1)] * 6 and tn_geometry(65) == (64, 2)
assert tn_geometry(1024) == (64, 16) and tn_geometry(1025) == (128, 9) and 1025 - 8 * 128 == 1
assert tn_geometry(1039) == (128, 9) and 1039 - 8 * 128 == 15

# past the caps: one case per kernel
FWD_CAP = 2048            # `cap = (2048 + nh - 1) / nh` workgroups in y, 4 tiles each (forward and dx launchers)
BWD_CAP = 16384 * 256     # `if (g > 16384) g = 16384` blocks of 256 threads (adjoint launcher)
BIG_FWD = dict(M=4115, H=4096)        # 258 row tiles against 4 * 64: tiles 256 and 257 on the second trip, the last of 3 rows
BIG_DX = dict(M=4115, Kd=4096)
BIG_BWD = dict(M=524307, H=128)       # 4 194 456 threads against 4 194 304: 152 of them take a second trip (19 rows)
assert -(-BIG_FWD["M"] // 16) == 258 > 4 * -(-FWD_CAP // (BIG_FWD["H"] // HD)) == 256 and BIG_FWD["M"] - 257 * 16 == 3
assert -(-BIG_DX["M"] // 16) > 4 * -(-FWD_CAP // (BIG_DX["Kd"] // 128))
assert BIG_BWD["M"] * (BIG_BWD["H"] // HD) * 8 > BWD_CAP
SLAB = 65536              # rows per float64 slab of the device-side reference


# ------------------------------------------------------------------------------------------------------------------ inputs
def ints(shape, lo, hi, seed, device="cpu"):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randint(lo, hi + 1, shape, generator=g, device=device).float()


def gauss(shape, seed, scale=1.0, device="cpu"):
    g = torch.Generator(device=device).manual_seed(seed)
    return torch.randn(shape, generator=g, device=device) * scale


def quarter_turns(T, device="cpu", nan_rows=2):
    """fp32 [T + nan_rows][128] = cos(64) | sin(64): a quarter turn per position and column pair, (cos, sin) in {(1, 0), (0, 1),
    (-1, 0), (0, -1)}, varying with both; then rows of NaN, so that a position read past T - 1 poisons the output"""
    pos, i = torch.arange(T, device=device)[:, None], torch.arange(64, device=device)[None, :]
    q = (3 * pos + 5 * i + i // 7) % 4
    co = torch.tensor([1.0, 0.0, -1.0, 0.0], device=device)[q]
    si = torch.tensor([0.0, 1.0, 0.0, -1.0], device=device)[q]
    return torch.cat([torch.cat([co, si], 1), torch.full((nan_rows, HD), NAN, device=device)], 0).contiguous()


def angle_table(T, nan_rows=2):
    """the trainer's table (base 10000) with the same NaN rows after row T - 1"""
    return torch.cat([rope_table(T, HD), torch.full((nan_rows, HD), NAN)], 0).contiguous()


def probe_weights(rows, width, device="cpu"):
    """[rows][width]: entry (global rank r, column c) = ((c mod 128) + 37 r) mod 251 - 125. Along a rank the 128 columns of a head
    differ, along a column the 24 ranks differ (37 r mod 251 is one-to-one), so a misplaced column or rank changes the entry. 24 x
    128 entries cannot all differ among the integers bf16 holds exactly; two entries agree only at a column distance of 37 (r' - r) mod
    251, which no index of the kernels produces."""
    r, c = torch.arange(rows, device=device)[:, None], torch.arange(width, device=device)[None, :]
    return (((c % HD) + 37 * r) % 251 - 125).float()


def one_hot_ranks(rows, M, device="cpu"):
    """t^T [rows][M]: row m of t is one-hot in rank m mod rows"""
    t = torch.zeros((rows, M), device=device)
    m = torch.arange(M, device=device)
    t[m % rows, m] = 1.0
    return t


SCALE_EXACT, SCALE_PROBE, SCALE_GAUSS = 2.0, 1.0, f32(2.0 / 0.7)
DROP_P = 0.3


def fwd_inputs(family, M, H, na, seed, dtype, device="cpu", k_only=False):
    """qkv [M][3H], tT [8 na][M], Bq, Bv, Bk [H][8] (Bk None for na = 2), scale.
    exact: qkv in [-8, 8], t in [-2, 2], B in [-3, 3], scale 2: an update is at most 2 * 8 * 2 * 3 = 96 (partial sums <= 48), the
    adapted value at most 104, and a quarter turn moves it without adding: every result <= 104.
    probe: t one-hot in rank m mod 8 na, B = probe_weights, scale 1: <= 8 + 125 = 133.
    k_only: the q and v rank rows of t^T are zero while Bq and Bv are not, so an update landing on the wrong operand shows."""
    if family == "gauss":
        qkv, tT = gauss((M, 3 * H), seed, device=device), gauss((8 * na, M), seed + 1, device=device)
        B = [gauss((H, 8), seed + 2 + a, 0.25, device=device) for a in range(na)]
        scale = SCALE_GAUSS
    else:
        qkv = ints((M, 3 * H), -8, 8, seed, device)
        if family == "probe":
            tT, w = one_hot_ranks(8 * na, M, device), probe_weights(8 * na, H, device)
            B = [w[8 * a:8 * a + 8].T.contiguous() for a in range(na)]
            scale = SCALE_PROBE
        else:
            tT = ints((8 * na, M), -2, 2, seed + 1, device)
            B = [ints((H, 8), -3, 3, seed + 2 + a, device) for a in range(na)]
            scale = SCALE_EXACT
    if k_only:
        assert na == 3
        tT[:16] = 0.0
    B = [b.to(dtype) for b in B] + [None] * (3 - na)
    return dict(qkv=qkv.to(dtype), tT=tT.to(dtype), Bq=B[0], Bv=B[1], Bk=B[2], scale=scale)


def bwd_inputs(family, M, H, seed, dtype, device="cpu"):
    """dq, dk, dv [M][H]; exact: integers in [-64, 64], which a quarter turn moves without adding"""
    mk = (lambda s: gauss((M, H), s, device=device)) if family == "gauss" else (lambda s: ints((M, H), -64, 64, s, device))
    return tuple(mk(seed + i).to(dtype) for i in range(3))


def dx_inputs(family, M, Kd, na, nmasks, seed, dtype, device="cpu"):
    """dtT [8 na][M], A [8 na][Kd], keeps (nmasks masks [M][Kd]), dx0 [M][Kd], scale.
    exact: dt in [-1, 1], A in [-2, 2], masks in {0, 1, 2}, dx0 in [-8, 8], scale 2: an adapter's product is at most 8 * 1 * 2 = 16
    (all 24 ranks in one MFMA: 48), masked 32, three of them 96, scaled 192, with dx0 200.
    probe: dt one-hot in rank m mod 8 na, A = probe_weights, scale 1, dx0 in [-6, 6]: <= 2 * 125 + 6 = 256.
    gauss: dt N(0, 1), A N(0, 1 / Kd), masks {0, 1 / (1 - p)} with p = 0.3, dx0 N(0, 1): the frozen product's adjoint."""
    if family == "gauss":
        dtT, A = gauss((8 * na, M), seed, device=device), gauss((8 * na, Kd), seed + 1, Kd ** -0.5, device=device)
        keeps = [(torch.rand((M, Kd), generator=torch.Generator(device=device).manual_seed(seed + 2 + i), device=device) >= DROP_P).float()
                 / (1.0 - DROP_P) for i in range(nmasks)]
        dx0, scale = gauss((M, Kd), seed + 5, device=device), SCALE_GAUSS
    else:
        keeps = [ints((M, Kd), 0, 2, seed + 2 + i, device) for i in range(nmasks)]
        if family == "probe":
            dtT, A, dx0, scale = one_hot_ranks(8 * na, M, device), probe_weights(8 * na, Kd, device), ints((M, Kd), -6, 6, seed + 5, device), SCALE_PROBE
        else:
            dtT, A = ints((8 * na, M), -1, 1, seed, device), ints((8 * na, Kd), -2, 2, seed + 1, device)
            dx0, scale = ints((M, Kd), -8, 8, seed + 5, device), SCALE_EXACT
    return dict(dtT=dtT.to(dtype), A=A.to(dtype), keeps=tuple(k.to(dtype) for k in keeps), dx0=dx0.to(dtype), scale=scale)


def tn_edge_rows(M):
    """the last row of every row block"""
    rpb, nb = tn_geometry(M)
    return [min((b + 1) * rpb, M) - 1 for b in range(nb)]


def tn_inputs(family, M, N, R, seed, dtype, device="cpu"):
    """sT [R][M], big [M][N], scale. exact: s in {-1, 0, 1} with two thirds of them zero, big in [-1, 1], scale 2; the last row of
    every row block and the columns 0 and N - 1 hold no zero, so that dropping one shows. A result is 2 * a sum of M terms of
    variance 2 / 9: about 30 at M = 1039. Its maximum is data, not a law, and is asserted at <= 256 where the inputs are made."""
    if family == "gauss":
        return dict(sT=gauss((R, M), seed, device=device).to(dtype), big=gauss((M, N), seed + 1, device=device).to(dtype), scale=SCALE_GAUSS)
    sT = ints((R, M), -1, 1, seed, device) * ints((R, M), 0, 1, seed + 1, device)
    big = ints((M, N), -1, 1, seed + 2, device)
    rows = torch.tensor(tn_edge_rows(M), device=device)
    sT[:, rows] = torch.where(sT[:, rows] == 0, torch.ones_like(sT[:, rows]), sT[:, rows])
    big[rows] = torch.where(big[rows] == 0, torch.ones_like(big[rows]), big[rows])
    if N > 1:     # column N - 1 differs from column 0 in every edge row
        big[rows, N - 1] = -big[rows, 0]
    out = SCALE_EXACT * (sT.double() @ big.double())
    assert float(out.abs().max()) <= EXACT_MAX, float(out.abs().max())
    return dict(sT=sT.to(dtype), big=big.to(dtype), scale=SCALE_EXACT)


def pad2d(x, rows, ld, fill, col0=0):
    """x [r][c] inside a [rows][ld] tensor of `fill`, as the view [:r, col0:col0 + c] of it"""
    r, c = x.shape
    full = torch.full((rows, ld), fill, dtype=x.dtype, device=x.device)
    full[:r, col0:col0 + c] = x
    return full


def embed(out, rows, ld, dtype, fill=SENT, clamp_row_written=False, skip_tile=None):
    """what a [rows][ld] buffer prefilled with `fill` holds after a kernel wrote `out` [M][W] into it. Two mistakes live here:
    the clamped row M - 1 (what the lanes past M compute) written into row M, and a 16-row tile never written."""
    M, W = out.shape
    full = torch.full((rows, ld), fill, dtype=dtype, device=out.device)
    full[:M, :W] = out.to(dtype)
    if clamp_row_written:
        full[M, :W] = full[M - 1, :W]
    if skip_tile is not None:
        full[16 * skip_tile:min(16 * skip_tile + 16, M), :W] = fill
    return full


# ----------------------------------------------------------------------------------------------------------- restatements
FWD_MISTAKES = ("k_after_rope",        # the k adapter's update added after k's rotation
                "v_from_q_rows",       # the v adapter's ranks read from the q rows of t^T
                "drop_rank",           # rank 3 of every adapter left out
                "partner32",           # the rotate-half partner taken at c +- 32
                "pos_div",             # position row / T
                "pos_mod_t1")          # position row % (T + 1)
BWD_MISTAKES = ("keep_sign",           # the forward's sin sign kept in the adjoint
                "partner32", "pos_div", "pos_mod_t1")
DX_MISTAKES = ("swap_qv", "swap_vk",   # masks exchanged
               "mask_wrong_ranks",     # keep_q applied to the v adapter's ranks as well
               "drop_rank",            # rank 3 of every adapter left out
               "no_k_lanes",           # the fh == 2 lanes (the k adapter) left out
               "ignore_accumulate",    # accumulate = 1 treated as 0, and 0 as 1 (adding what the destination was prefilled with)
               "skip_tile",            # one 16-row tile never written
               "double_tile")          # one 16-row tile accumulated twice
TN_MISTAKES = ("drop_block_last",      # the last row of every row block left out
               "double_block_last",    # ... counted twice
               "last_col_from_0")      # column N - 1 taken from column 0 (the clamp `colc` applied one column early)


def _flags(names, wrong):
    assert set(wrong) <= set(names), wrong
    f = dict.fromkeys(names, False)
    f.update(wrong)
    return f


def _rot(x, cs, T, adjoint, dt, row0=0, partner32=False, keep_sign=False, pos_div=False, pos_mod_t1=False, absolute=False):
    """rotate-half RoPE of x [M][H] per 128-column head at position (row0 + row) % T: with c the column inside the head,
    out[c] = x[c] cos[c % 64] - x[c + 64] sin[c % 64] for c < 64 and x[c] cos[c % 64] + x[c - 64] sin[c % 64] for c >= 64; the
    adjoint is the transpose (sin -> -sin). absolute: the sum of the absolute values of the two terms."""
    M, H = x.shape
    dev = x.device
    row = row0 + torch.arange(M, device=dev)
    pos = (row // T) if pos_div else row % (T + 1 if pos_mod_t1 else T)
    pos = pos.clamp_max(cs.shape[0] - 1)
    c = torch.arange(HD, device=dev)
    half = 32 if partner32 else 64
    low = (c % (2 * half)) < half
    partner = torch.where(low, c + half, c - half)
    sgn = torch.where(low, -1.0, 1.0).to(dt)
    if adjoint and not keep_sign:
        sgn = -sgn
    tab = cs.to(dt)[pos]
    co, si = tab[:, c % 64][:, None, :], tab[:, 64 + c % 64][:, None, :]
    v = x.to(dt).reshape(M, H // HD, HD)
    if absolute:
        return (v.abs() * co.abs() + v.abs()[..., partner] * si.abs()).reshape(M, H)
    return (v * co + sgn * v[..., partner] * si).reshape(M, H)


def qkv_rope_fwd(qkv, tT, Bq, Bv, Bk, cs, T, H, scale, dt=F64, row0=0, absolute=False, **wrong):
    """q = rope(qkv[:, :H] + scale t_q Bq^T), k = rope(qkv[:, H:2H] (+ scale t_k Bk^T)), v = qkv[:, 2H:] + scale t_v Bv^T; t_q, t_v,
    t_k = rows 0-7, 8-15, 16-23 of tT, transposed. qkv and tT hold the rows row0 .. row0 + M of the problem. The update is added
    before the rotation. absolute: the sums of the absolute values of the terms of q, k, v."""
    fl = _flags(FWD_MISTAKES, wrong)
    M = qkv.shape[0]
    s = abs(f32(scale)) if absolute else f32(scale)
    prep = (lambda z: z.to(dt).abs()) if absolute else (lambda z: z.to(dt))
    t, x = prep(tT[:, :M]), prep(qkv[:, :3 * H])
    if fl["drop_rank"]:
        t = t.clone()
        t[3::8] = 0.0
    tq, tv = t[0:8], (t[0:8] if fl["v_from_q_rows"] else t[8:16])
    q = x[:, :H] + s * (tq.T @ prep(Bq).T)
    k = x[:, H:2 * H]
    v = x[:, 2 * H:] + s * (tv.T @ prep(Bv).T)
    uk = None if Bk is None else s * (t[16:24].T @ prep(Bk).T)
    if uk is not None and not fl["k_after_rope"]:
        k = k + uk
    kw = dict(row0=row0, partner32=fl["partner32"], pos_div=fl["pos_div"], pos_mod_t1=fl["pos_mod_t1"], absolute=absolute)
    q, k = _rot(q, cs, T, False, dt, **kw), _rot(k, cs, T, False, dt, **kw)
    if uk is not None and fl["k_after_rope"]:
        k = k + uk
    return q, k, v


def qkv_rope_fwd_ordered(qkv, tT, Bq, Bv, Bk, cs, T, H, scale, dtype):
    """The same three results, correct, in the kernel's own order: fp32, the ranks added one after the other from zero (the k index
    of the MFMA), then scale *, then the add, then the rotation, rounded to the 16-bit type once. Not a reference: the second
    evaluation that shows the bound can be met."""
    M, s = qkv.shape[0], torch.tensor(f32(scale), dtype=F32)
    t, x = tT[:, :M].float(), qkv[:, :3 * H].float()

    def upd(a, B):
        acc = torch.zeros((M, H))
        for j in range(8):
            acc = acc + t[8 * a + j][:, None] * B.float()[:, j][None, :]
        return s * acc
    q, k, v = x[:, :H] + upd(0, Bq), x[:, H:2 * H], x[:, 2 * H:] + upd(1, Bv)
    if Bk is not None:
        k = k + upd(2, Bk)
    return tuple(z.to(dtype) for z in (_rot(q, cs, T, False, F32), _rot(k, cs, T, False, F32), v))


def qkv_rope_bwd(dq, dk, dv, cs, T, H, dt=F64, row0=0, absolute=False, **wrong):
    """dqkv [M][3H] = [rope^T dq | rope^T dk | dv]: the transpose of the forward's rotation; dv is copied"""
    fl = _flags(BWD_MISTAKES, wrong)
    kw = dict(row0=row0, absolute=absolute, **fl)
    v = dv[:, :H].to(dt)
    return torch.cat([_rot(dq[:, :H], cs, T, True, dt, **kw), _rot(dk[:, :H], cs, T, True, dt, **kw), v.abs() if absolute else v], 1)


def dx(dtT, A, keeps, dx0, scale, na, dt=F64, tile=None, prefill=NAN, absolute=False, **wrong):
    """dx [M][Kd] = (dx0 +) scale * sum over the na adapters of keep_a o (dt_a . A_a), dt_a = rows 8a .. 8a + 7 of dtT transposed,
    A_a the same rows of A. keeps: () no mask, (keep,) one mask for every adapter, (keep_q, keep_v) with na = 2, (keep_q, keep_v,
    keep_k) with na = 3. dx0 None: accumulate = 0. In the kernel's order: without a mask or with one, all ranks in one sum, then
    scale *, then the mask; with more, scale * (q + v), then + scale * k; then + dx0. `tile`: the 16-row tile the two tile mistakes
    hit (default: the last); `prefill`: what the destination held where accumulate = 0."""
    fl = _flags(DX_MISTAKES, wrong)
    M, Kd = dtT.shape[1], A.shape[1]
    s = abs(f32(scale)) if absolute else f32(scale)
    prep = (lambda z: z.to(dt).abs()) if absolute else (lambda z: z.to(dt))
    d, a = prep(dtT[:8 * na]), prep(A[:8 * na])
    if fl["drop_rank"]:
        d = d.clone()
        d[3::8] = 0.0
    P = [d[8 * i:8 * i + 8].T @ a[8 * i:8 * i + 8] for i in range(na)]
    if fl["no_k_lanes"] and na == 3:
        P[2] = torch.zeros_like(P[2])
    ks = [prep(k[:M, :Kd]) for k in keeps]
    assert len(ks) in (0, 1, na), (len(ks), na)
    if len(ks) >= 2 and fl["swap_qv"]:
        ks[0], ks[1] = ks[1], ks[0]
    if len(ks) == 3 and fl["swap_vk"]:
        ks[1], ks[2] = ks[2], ks[1]
    if len(ks) >= 2 and fl["mask_wrong_ranks"]:
        ks[1] = ks[0]
    if len(ks) <= 1:
        u = s * sum(P[1:], P[0])
        if ks:
            u = u * ks[0]
    else:
        u = s * (P[0] * ks[0] + P[1] * ks[1])
        if len(ks) == 3:
            u = u + s * (P[2] * ks[2])
    old = None if dx0 is None else prep(dx0[:M, :Kd])
    if fl["ignore_accumulate"]:
        out = u.clone() if old is not None else u + prefill
    else:
        out = u + old if old is not None else u.clone()
    if fl["skip_tile"] or fl["double_tile"]:
        tile = (M - 1) // 16 if tile is None else tile
        r = slice(16 * tile, min(16 * tile + 16, M))
        if fl["skip_tile"]:
            out[r] = old[r] if old is not None else prefill
        else:
            out[r] = out[r] + u[r] if old is not None else out[r]     # without accumulate a second pass writes the same values
    return out


def dx_ordered(dtT, A, keeps, dx0, scale, na, dtype):
    """dx, correct, in the kernel's order in fp32: the ranks one after the other from zero, per adapter where the masks differ"""
    M, Kd = dtT.shape[1], A.shape[1]
    s = torch.tensor(f32(scale), dtype=F32)
    d, a = dtT.float(), A.float()

    def prod(rows):
        acc = torch.zeros((M, Kd))
        for r in rows:
            acc = acc + d[r][:, None] * a[r][None, :]
        return acc
    ks = [k[:M, :Kd].float() for k in keeps]
    if len(ks) <= 1:
        u = s * prod(range(8 * na))
        if ks:
            u = u * ks[0]
    else:
        u = s * (prod(range(0, 8)) * ks[0] + prod(range(8, 16)) * ks[1])
        if len(ks) == 3:
            u = u + s * (prod(range(16, 24)) * ks[2])
    return (u if dx0 is None else u + dx0[:M, :Kd].float()).to(dtype)


def lora_tn(sT, big, M, scale, j_valid, transposed, dt=F64, N=None, absolute=False, **wrong):
    """out = scale * sT[:j_valid, :M] . big[:M, :N], [j_valid][N] or transposed [N][j_valid]. fp32: one product per row block, the
    blocks added in index order, then scale *."""
    fl = _flags(TN_MISTAKES, wrong)
    N = big.shape[1] if N is None else N
    prep = (lambda z: z.to(dt).abs()) if absolute else (lambda z: z.to(dt))
    s, b = prep(sT[:j_valid, :M]), prep(big[:M, :N])
    rpb, nb = tn_geometry(M)
    if dt == F64:
        out = s @ b
    else:
        out = torch.zeros((j_valid, N), dtype=dt, device=b.device)
        for i in range(nb):
            out = out + s[:, i * rpb:(i + 1) * rpb] @ b[i * rpb:(i + 1) * rpb]
    if fl["drop_block_last"] or fl["double_block_last"]:
        rows = tn_edge_rows(M)
        out = out + (-1.0 if fl["drop_block_last"] else 1.0) * (s[:, rows] @ b[rows])
    if fl["last_col_from_0"]:
        out = out.clone()
        out[:, N - 1] = out[:, 0]
    out = (abs(f32(scale)) if absolute else f32(scale)) * out
    return out.T if transposed else out


def lora_tn_ordered(sT, big, M, scale, j_valid, out_dtype, N=None):
    """lora_tn [j_valid][N], correct, in the kernel's order in fp32: inside a row block wave w takes the 16-row steps w, w + 4, ...
    one row after the other (a step's products are fused multiply-adds into the wave's sum: emulated in float64 per step, rounded
    to fp32 per row), the four waves meet as ((w0 + w1) + w2) + w3, the blocks are added in index order from zero, then scale *."""
    N = big.shape[1] if N is None else N
    s, b = sT[:j_valid, :M].float(), big[:M, :N].float()
    rpb, nb = tn_geometry(M)
    total = torch.zeros((j_valid, N))
    for blk in range(nb):
        lo, hi = blk * rpb, min((blk + 1) * rpb, M)
        waves = []
        for w in range(4):
            acc = torch.zeros((j_valid, N))
            for m0 in range(lo + 16 * w, hi, 64):
                for m in range(m0, min(m0 + 16, hi)):
                    acc = (acc.double() + s[:, m].double()[:, None] * b[m].double()[None, :]).float()
            waves.append(acc)
        total = total + (((waves[0] + waves[1]) + waves[2]) + waves[3])
    return (total * torch.tensor(f32(scale), dtype=F32)).to(out_dtype)


# ------------------------------------------------------------------------------------------------------------------ bounds
def expect(fn, args, dtypes, **kw):
    """[(float64 reference, elementwise bound)] per output of fn(*args, **kw): K times the worst error of the fp32 evaluation
    against float64, FLOOR_ULPS fp32 ulps of the sum of the absolute values of the output's terms (fn(..., absolute=True)), half a
    storage ulp (none for an fp32 output)"""
    ref, ev, ab = fn(*args, dt=F64, **kw), fn(*args, dt=F32, **kw), fn(*args, dt=F64, absolute=True, **kw)
    if not isinstance(ref, tuple):
        ref, ev, ab, dtypes = (ref,), (ev,), (ab,), (dtypes,)
    return [(r, bound(r, e, d, scale=a)) for r, e, a, d in zip(ref, ev, ab, dtypes)]


def old_criterion(got, ref):
    """what the node-level tests assert today: max |got - ref| <= 3e-2 max |ref| (False for a non-finite result)"""
    got, ref = got.double(), ref.double()
    return bool(torch.isfinite(got).all()) and float((got - ref).abs().max()) <= OLD_TOL * float(ref.abs().max())
