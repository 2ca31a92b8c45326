"""CPU restatement of the NF4 format (bitsandbytes' load_in_4bit, nf4, fp16 compute; see haff/quant.py's docstring), written
independently of the product for the tests: quantise / dequantise one f16 weight tensor in torch on the CPU."""
import torch

NF4 = torch.tensor([-1.0, -0.6961928009986877, -0.5250730514526367, -0.39491748809814453, -0.28444138169288635,
                    -0.18477343022823334, -0.09105003625154495, 0.0, 0.07958029955625534, 0.16093020141124725,
                    0.24611230194568634, 0.33791524171829224, 0.44070982933044434, 0.5626170039176941, 0.7229568362236023,
                    1.0], dtype=torch.float32)


def dynamic_map():
    """create_dynamic_map(signed=True, max_exponent_bits=7, total_bits=8): 7 non-sign bits, no extra items; decade i = 0..6 holds
    the 2^i midpoints of linspace(0.1, 1, 2^i + 1) scaled by 10^(-6 + i), positive and negative; then 0 and 1.0; sorted."""
    vals = [0.0, 1.0]
    for i in range(7):
        pts = torch.linspace(0.1, 1, 2 ** i + 1)
        mids = (pts[:-1] + pts[1:]) / 2.0
        scale = 10 ** (-6 + i)
        vals += (scale * mids).tolist() + (-scale * mids).tolist()
    return torch.tensor(sorted(vals), dtype=torch.float32)


def _nearest(x, table):
    """number of fp32 midpoints of neighbouring table values strictly below x (a midpoint value takes the lower index)"""
    mids = (table[:-1] + table[1:]) * 0.5
    return torch.bucketize(x, mids, right=False)


def _inv(a):
    return torch.where(a > 0, 1.0 / torch.where(a > 0, a, torch.ones_like(a)), torch.zeros_like(a))


def quantize(w16, double_quant=True, offset=None):
    """w16 f16 [N, K] (K % 64 == 0) -> (packed uint8 [N, K/2], dequantised absmax f32 [N, K/64], offset f32). offset: the mean
    of the absmax values to use (None: the float64 mean rounded to fp32)."""
    N, K = w16.shape
    w = w16.float().reshape(-1, 64)
    amax = w.abs().amax(1)
    codes = _nearest(w * _inv(amax)[:, None], NF4).to(torch.uint8).reshape(N, K)
    packed = (codes[:, 0::2] << 4) | codes[:, 1::2]
    if offset is None:
        offset = torch.tensor(amax.double().mean().item(), dtype=torch.float32)
    offset = torch.as_tensor(offset, dtype=torch.float32).reshape(())
    if double_quant:
        d = amax - offset
        nb = d.numel()
        pad = (-nb) % 256
        dp = torch.cat([d, torch.zeros(pad)]).reshape(-1, 256)
        a2 = dp.abs().amax(1)
        c = _nearest(dp * _inv(a2)[:, None], dynamic_map())
        amax = ((dynamic_map()[c] * a2[:, None]) + offset).reshape(-1)[:nb]
    return packed, amax.reshape(N, K // 64), offset


def dequant(packed, absmax):
    """f16 [N, K] = f16_rn(NF4[code] * absmax)"""
    N = packed.shape[0]
    codes = torch.stack([packed >> 4, packed & 15], dim=2).reshape(N, -1).long()
    return (NF4[codes].reshape(N, -1, 64) * absmax[:, :, None]).reshape(N, -1).half()


# The tolerance of the NF4 product against product() below: C_ACC * (sum_k |x w| + |bias|), plus the output's rounding.
# haff_gemm_nf4_f16 multiplies f16 x by f16 weights (exact in fp32) and accumulates in fp32: each of its 8 waves chains two
# v_mfma_f32_16x16x32_f16 per 64-block of its K range, then the 8 partial sums are added in wave order and the bias added. At the
# largest K the model runs (13824: 216 blocks, 27 per wave) that is 54 MFMAs, 7 adds and the bias: counting two roundings per MFMA
# (its internal sum, then the add into the accumulator) and each rounding as a whole fp32 ulp (2^-23, which holds for a
# truncating adder as much as for round to nearest), the error is below (2 * 54 + 8) * 2^-23 = 1.38e-5 of sum |x w| + |bias|.
# C_ACC = 2^-16 (1.53e-5) is that bound rounded up to a power of two. tests/test_nf4_cpu.py shows that it still rejects one
# dropped 64-block, a neighbouring block's absmax, a row shift inside a weight tile and a wrong row of an activation tile.
C_ACC = 2.0 ** -16


def product(x16, packed, absmax, bias=None):
    """float64 [M, N] = x16 [M, K] (f16 values) @ dequant(packed, absmax).T (+ bias): the NF4 product without any rounding but the
    weights' own f16_rn(NF4[code] * absmax)."""
    w = dequant(packed, absmax).double()
    y = x16.double() @ w.T
    return y if bias is None else y + bias.double()[None, :]


def magnitude(x, wdeq, bias=None):
    """float64 [M, N] = sum_k |x w| (+ |bias|): the scale of the accumulation error."""
    m = x.double().abs() @ wdeq.double().abs().T
    return m if bias is None else m + bias.double().abs()[None, :]


def tol(x, wdeq, bias, out_dtype, ref=None):
    """float64 [M, N]: how far the NF4 product (f16 x [M, K], dequantised weights [N, K], fp32 bias or None) may lie from product():
    C_ACC * magnitude, plus one ulp of the output format at |ref| (ref: the reference output values; None: no output rounding)."""
    t = C_ACC * magnitude(x, wdeq, bias)
    if ref is not None:
        r = ref.double().abs()
        t = t + (r.clamp_min(2.0 ** -14) * 2.0 ** -10 if out_dtype == torch.float16 else r * 2.0 ** -23)
    return t
