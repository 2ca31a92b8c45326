"""CPU restatement of the two kernels that serve LoRA adapters unmerged on NF4 weights (csrc/gemm_nf4.hip), on top of nf4_ref and
written independently of the product:

  dequant_lora  haff_nf4_dequant_lora_f16, bit for bit: every operation is one fp32 operation of torch on the CPU, in the order the
                header fixes (d = NF4[code] * absmax; u += B[n, j] * A[8 seg(n) + j, k] for j = 0..7, the product exact in fp32;
                out = f16_rn(d + s * u)).
  product_lora  haff_gemm_nf4_lora_f16 in float64 without any rounding but the weights' own and t's: x deq(W)^T +
                s * sum_j t[m, 8 seg(n) + j] * B[n, j] (+ bias).

Layout: a fused weight has nseg row segments of seg_rows stored rows, seg(n) = (n // seg_rows) % nseg; a_cat f16 [8 nseg, K]; b f16
[N, 8] in the stored row order; t = f16(x a_cat^T) [M, 8 nseg]."""
import math

import torch

import nf4_ref as R


def seg_of(N, nseg, seg_rows):
    return (torch.arange(N) // seg_rows) % nseg


def rank_rows(N, nseg, seg_rows):
    """int64 [N, 8]: the rows of a_cat (= the columns of t) stored row n reads."""
    return 8 * seg_of(N, nseg, seg_rows)[:, None] + torch.arange(8)[None, :]


def dequant_lora(packed, absmax, a_cat, b, nseg, seg_rows, scale):
    """f16 [N, K], the bits haff_nf4_dequant_lora_f16 writes."""
    N = packed.shape[0]
    codes = torch.stack([packed >> 4, packed & 15], dim=2).reshape(N, -1).long()
    d = (R.NF4[codes].reshape(N, -1, 64) * absmax[:, :, None]).reshape(N, -1)          # fp32, one rounding
    rows = rank_rows(N, nseg, seg_rows)
    a32, b32 = a_cat.float(), b.float()
    u = torch.zeros_like(d)
    for j in range(8):
        u = u + b32[:, j:j + 1] * a32[rows[:, j]]       # f16 x f16 is exact in fp32; the add rounds once
    su = torch.tensor(scale, dtype=torch.float32) * u
    return (d + su).half()


def rank_values(x16, a_cat):
    """t = f16_rn(x a_cat^T) [M, 8 nseg] (float64 sum, one rounding)."""
    return (x16.double() @ a_cat.double().T).half()


def update(t16, b, nseg, seg_rows, scale):
    """float64 [M, N] = s * sum_j t[m, 8 seg(n) + j] * B[n, j]"""
    rows = rank_rows(b.shape[0], nseg, seg_rows)
    return scale * torch.einsum("mnj,nj->mn", t16.double()[:, rows], b.double())


def update_magnitude(t16, b, nseg, seg_rows, scale):
    """float64 [M, N] = |s| * sum_j |t B|: the scale of the rank update's accumulation error."""
    rows = rank_rows(b.shape[0], nseg, seg_rows)
    return abs(scale) * torch.einsum("mnj,nj->mn", t16.double().abs()[:, rows], b.double().abs())


def product_lora(x16, packed, absmax, t16, b, nseg, seg_rows, scale, bias=None):
    return R.product(x16, packed, absmax, bias) + update(t16, b, nseg, seg_rows, scale)


# haff_gemm_nf4_lora_f16 adds to the plain product's fp32 sum ONE more v_mfma_f32_16x16x32_f16 (8 live products of t and B, exact in
# fp32), one multiply by s and one add: four roundings at most, each below an fp32 ulp of a partial result that sum_j |t B| (times s)
# bounds. nf4_ref.C_ACC = 2^-16 covers 116 such roundings of the plain product; the same constant on the update's magnitude is more
# than its four need, and test_lora_serve_cpu.py shows it still rejects the mistakes this kernel can make.
def tol(x16, wdeq, bias, out_dtype, t16, b, nseg, seg_rows, scale, ref=None):
    return R.tol(x16, wdeq, bias, out_dtype, ref) + R.C_ACC * update_magnitude(t16, b, nseg, seg_rows, scale)


def make_case(M, N, K, nseg, seg_rows, seed, r=8, scale=2.0, zero_seg=None):
    """Inputs with train_model.init_lora(init_b_zero=False)'s distributions: A ~ U(+-1/sqrt(K)), B ~ U(+-0.05); x ~ N(0, 1),
    W ~ N(0, 0.02). Rank r < 8 is zero-padded; zero_seg: a segment without adapter (its a_cat rows and its rows of b zero)."""
    g = torch.Generator().manual_seed(seed)
    w = (torch.randn(N, K, generator=g) * 0.02).half()
    x = torch.randn(M, K, generator=g).half()
    packed, absmax, _ = R.quantize(w)
    a_cat = torch.zeros(8 * nseg, K)
    for s in range(nseg):
        a_cat[8 * s:8 * s + r] = (torch.rand((r, K), generator=g) * 2 - 1) / math.sqrt(K)
    b = torch.zeros(N, 8)
    b[:, :r] = (torch.rand((N, r), generator=g) * 2 - 1) * 0.05
    if zero_seg is not None:
        a_cat[8 * zero_seg:8 * zero_seg + 8] = 0
        b[seg_of(N, nseg, seg_rows) == zero_seg] = 0
    a_cat, b = a_cat.half(), b.half()
    return {"x": x, "packed": packed, "absmax": absmax, "wdeq": R.dequant(packed, absmax), "a_cat": a_cat, "b": b,
            "t": rank_values(x, a_cat), "nseg": nseg, "seg_rows": seg_rows, "scale": scale}
