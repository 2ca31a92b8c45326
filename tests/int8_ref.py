"""An independent CPU restatement of LLM.int8 as the 8-bit load applies it (bitsandbytes 0.41.1 MatMul8bitLt, threshold 6.0, no fp16
weight copy), written from the rules in 2handedafforder_amd/quant.py's int8 section with numpy only — it shares no code with the
package. Everything is float32 numpy arithmetic with one rounding per operation; rint is numpy's round half to even.

Segments: rows [s * seg_rows, (s + 1) * seg_rows) are one frame; its first valid[s] rows decide its outlier columns. masks (bool
[S, K]) are ORed into in place when given: a frame's sticky masks across KV-cached decode steps."""
import numpy as np

C = np.float32(6.200012e-05)
F127 = np.float32(127.0)


def _f16(x):
    return np.asarray(x, dtype=np.float32).astype(np.float16).astype(np.float32)


def quantize_weight(w):
    """w [N, K] (any float) -> (CB int8 [N, K], SCB float32 [N]); w is rounded to fp16 first."""
    w = _f16(np.asarray(w, dtype=np.float32))
    scb = np.max(np.abs(w), axis=1).astype(np.float32)
    cb = np.zeros(w.shape, dtype=np.int8)
    for n in range(w.shape[0]):
        if scb[n] > 0:
            s = np.float32(F127 / scb[n])
            cb[n] = np.rint(w[n] * s).astype(np.int8)
    return cb, scb


def quantize_rows(a, threshold, seg_rows=None, valid=None, masks=None):
    """a [M, K] fp16 values -> (CA int8 [M, K], SCA float32 [M], masks bool [S, K])."""
    a = _f16(np.asarray(a, dtype=np.float32))
    M, K = a.shape
    seg_rows = M if seg_rows is None else seg_rows
    S = -(-M // seg_rows)
    thr = np.float32(threshold)
    if masks is None:
        masks = np.zeros((S, K), dtype=bool)
    own = np.abs(a) >= thr if thr > 0 else np.zeros(a.shape, dtype=bool)
    for m in range(M):
        s, r = divmod(m, seg_rows)
        if valid is None or r < int(valid[s]):
            masks[s] |= own[m]
    sca = np.zeros(M, dtype=np.float32)
    ca = np.zeros((M, K), dtype=np.int8)
    for m in range(M):
        keep = ~own[m]
        sca[m] = np.max(np.abs(a[m][keep])) if keep.any() else np.float32(0)
        if sca[m] > 0:
            s = np.float32(F127 / sca[m])
            q = np.rint(a[m] * s)
            q[own[m] | masks[m // seg_rows]] = 0
            ca[m] = q.astype(np.int8)
    return ca, sca, masks


def product(a, ca, sca, cb, scb, masks, seg_rows=None, bias=None):
    """Y f16 [M, N]: the dequantised int32 product, then the fixed-order outlier sum of the row's segment columns."""
    a = _f16(np.asarray(a, dtype=np.float32))
    M = a.shape[0]
    seg_rows = M if seg_rows is None else seg_rows
    acc = ca.astype(np.float64) @ cb.astype(np.float64).T        # integer sums below 2^53: exact in float64
    assert np.abs(acc).max(initial=0) < 2 ** 31
    t = acc.astype(np.float32)
    t = (t * C).astype(np.float32)
    t = (t * sca[:, None]).astype(np.float32)
    t = (t * scb[None, :]).astype(np.float32)
    if bias is not None:
        t = (t + np.asarray(bias, dtype=np.float32)[None, :]).astype(np.float32)
    y = _f16(t)
    for s in range(masks.shape[0]):
        cols = np.flatnonzero(masks[s])
        rows = slice(s * seg_rows, min(M, (s + 1) * seg_rows))
        if cols.size == 0:
            continue
        sub_b = _f16((cb[:, cols].astype(np.float32) * scb[:, None]) / F127)   # [N, n]
        o = np.zeros((a[rows].shape[0], cb.shape[0]), dtype=np.float32)
        for j, c in enumerate(cols):                                             # ascending columns, one rounding per add
            o = (o + a[rows, c][:, None] * sub_b[None, :, j]).astype(np.float32)
        y[rows] = _f16(y[rows] + _f16(o))
    return y.astype(np.float16)


def linear(a, w_cb, w_scb, threshold, seg_rows=None, valid=None, masks=None, bias=None):
    """One converted Linear on fp16 rows a: quantise the rows, then the product -> f16 [M, N]."""
    ca, sca, masks = quantize_rows(a, threshold, seg_rows, valid, masks)
    return product(a, ca, sca, w_cb, w_scb, masks, seg_rows, bias)


ACT_NONE, ACT_GELU, ACT_QUICK_GELU, ACT_RELU, ACT_SILU = 0, 1, 2, 3, 4
EXACT_ACTS = (ACT_NONE, ACT_RELU)   # the epilogues below that are bit-exact; the others use the device's erff / __expf / rcpf


def _erf(x):
    import math
    return np.vectorize(math.erf, otypes=[np.float64])(x)


def _act(v, act):
    """act of fp32 values v: ACT_NONE / ACT_RELU exactly in fp32, the others in float64 (the exact function of the fp32 input)."""
    if act == ACT_NONE:
        return v
    if act == ACT_RELU:
        return np.maximum(v, np.float32(0))
    x = v.astype(np.float64)
    if act == ACT_GELU:
        return 0.5 * x * (1.0 + _erf(x * 0.7071067811865476))
    if act == ACT_QUICK_GELU:
        return x / (1.0 + np.exp(-1.702 * x))
    if act == ACT_SILU:
        return x / (1.0 + np.exp(-x))
    raise ValueError(f"unknown act {act}")


def swiglu_split(y):
    """(gate, up) columns of a [.., N] product whose weight rows are interleaved [gate x16 | up x16] -> two [.., N/2]."""
    t = np.asarray(y).reshape(*np.shape(y)[:-1], -1, 2, 16)
    return t[..., 0, :].reshape(*np.shape(y)[:-1], -1), t[..., 1, :].reshape(*np.shape(y)[:-1], -1)


def epilogue(y, act=ACT_NONE, resid=None, out_f32=False, row_map=None, swiglu=False, out=None):
    """The int8 product's epilogue (gemm_int8.hip i8_epilogue) on the f16 Y that product() returns: act (or SwiGLU of the interleaved
    gate / up columns) of the f16-valued Y in fp32, + resid (indexed like the output) in fp32, stored as f16 (round to nearest even)
    or fp32, row m to output row row_map[m] (-1: not written). out: the output's contents before the call (rows the map does not
    write keep them; None: zeros of [M, n_out]). Returns the new output (float16 or float32).

    ACT_NONE / ACT_RELU without SwiGLU are exact restatements. GELU, quick-GELU, SiLU and SwiGLU are evaluated in float64 from the
    same fp32 inputs, then rounded once to fp32: the device's erff / __expf / rcpf differ from them by a few fp32 ulps."""
    y = np.asarray(y).astype(np.float32)
    if swiglu:
        g, u = swiglu_split(y)
        g64 = g.astype(np.float64)
        v = (g64 / (1.0 + np.exp(-g64)) * u.astype(np.float64)).astype(np.float32)
    else:
        v = np.asarray(_act(y, act)).astype(np.float32)
    M, n_out = v.shape
    odt = np.float32 if out_f32 else np.float16
    res = np.zeros((M, n_out), dtype=odt) if out is None else np.array(out, dtype=odt)
    rows = np.arange(M) if row_map is None else np.asarray(row_map)
    for m in range(M):
        r = int(rows[m])
        if r < 0:
            continue
        t = v[m]
        if resid is not None:
            t = (t + np.asarray(resid, dtype=np.float32)[r]).astype(np.float32)
        res[r] = t.astype(odt)
    return res
