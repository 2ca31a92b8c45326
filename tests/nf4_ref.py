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
