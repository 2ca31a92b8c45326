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
