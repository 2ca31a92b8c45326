"""Tensor-level wrappers over the C-ABI of libhaff_hip.so.

torch is used here only for device memory and the current HIP stream; every arithmetic op below is a
hand-written HIP kernel. All functions require CUDA(HIP) tensors and raise if the library is missing.
dtype policy: torch.bfloat16 = throughput mode (bf16 MFMA, fp32 accumulate), torch.float32 = parity mode, torch.float16 = the
fp16 inference mode (f16 MFMA, fp32 accumulate: the *_f16 instances of the 16-bit kernels, dtype code 3 elsewhere).
"""
import ctypes

import numpy as np
import torch

from .lib import check, load_library

ACT_NONE, ACT_GELU, ACT_QUICK_GELU, ACT_RELU, ACT_SILU = 0, 1, 2, 3, 4


def _dt(t):
    if t.dtype == torch.bfloat16:
        return 0
    if t.dtype == torch.float32:
        return 1
    if t.dtype == torch.float16:
        return 3
    raise TypeError(f"unsupported dtype {t.dtype}")


def _fn(lib, name, dtype, f32=False):
    """The entry point of the operand format: haff_*_bf16 for bf16, its haff_*_f16 sibling for fp16 (same arguments) and, in a
    family that has one (f32=True), the haff_*_f32 sibling for every other dtype."""
    if dtype == torch.float16:
        name = name.replace("_bf16", "_f16")
    elif f32 and dtype != torch.bfloat16:
        name = name.replace("_bf16", "_f32")
    return getattr(lib, name)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return 0 if t is None else t.data_ptr()


def _req(t, name):
    if not t.is_cuda:
        raise RuntimeError(f"{name} must live in HBM (cuda tensor); the hot path has no CPU fallback")


_WORKSPACES = {}


def _workspace(device, nbytes):
    """Scratch HBM for kernels that take a caller-provided workspace: one buffer per (device, stream), so launches on
    different HIP streams never share one.
    Under hipGraph capture the key is the CAPTURE stream: the buffer is then allocated from the graph's pool and its address is
    baked into the graph. Branches of one capture that fork onto other streams get their own buffers (their own keys), but two
    different graphs may end up holding the same buffer — which is why LisaMI355 replays its graphs one after another on one
    stream (lisa.py: `_graph_pool`, "replays never overlap") and never replays one beside an eager launch that uses the
    workspace of the same stream key. A caller that wants concurrent replays must capture them with distinct workspaces."""
    key = (device.index, _stream())
    buf = _WORKSPACES.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = _WORKSPACES[key] = torch.empty((nbytes,), dtype=torch.uint8, device=device)
    return buf


def _out(out, shape, dtype, device):
    """A wrapper's output: a new tensor, or the caller's, which must be exactly that one (and contiguous)."""
    if out is None:
        return torch.empty(tuple(shape), dtype=dtype, device=device)
    assert out.dtype == dtype and out.is_contiguous() and tuple(out.shape) == tuple(shape) and out.device == device, (out.dtype, out.shape)
    return out


def _linear_out(x, M, N, swiglu, out, out_rows, out_dtype, resid, bias, row_map):
    """The output of a linear*(): the caller's `out`, or a new [out_rows or M, N (SwiGLU: N / 2)] tensor of out_dtype (None: x's), and
    the epilogue's operands checked against it: resid like out, bias fp32 [N], row_map int32 [M]."""
    n_out = N // 2 if swiglu else N
    if out is None:
        out = torch.empty((M if out_rows is None else out_rows, n_out), dtype=x.dtype if out_dtype is None else out_dtype, device=x.device)
    assert out.stride(1) == 1 and out.shape[1] == n_out
    if resid is not None:
        assert resid.dtype == out.dtype and resid.stride(1) == 1
    if bias is not None:
        assert bias.dtype == torch.float32 and bias.numel() == N
    if row_map is not None:
        assert row_map.dtype == torch.int32 and row_map.numel() == M
    return out


def _epilogue_args(out, bias, resid, row_map, M, N, K, act, swiglu):
    """The ten arguments `bias, resid, ldr, row_map, M, N, K, act, out_f32, swiglu` that follow `C, ldc` in every product's C signature"""
    return (_p(bias), _p(resid), 0 if resid is None else resid.stride(0), _p(row_map), M, N, K, act,
            1 if out.dtype == torch.float32 else 0, 1 if swiglu else 0)


def upload_pinned(array, device):
    """A numpy array as a device tensor, through a pinned staging copy: the upload does not block the host."""
    return torch.from_numpy(np.ascontiguousarray(array)).pin_memory().to(device, non_blocking=True)


def row_stats(x, eps, rms=False):
    """Per-row {mean, rstd} (rms: {0, rsqrt(mean(x^2)+eps)}) as fp32 [rows, 2] — the normalisation itself is applied
    by linear(..., ln_stats=, ln_colsum=)."""
    lib = load_library()
    _req(x, "x")
    assert x.dim() == 2 and x.stride(1) == 1
    stats = torch.empty((x.shape[0], 2), dtype=torch.float32, device=x.device)
    rc = lib.haff_row_stats(x.data_ptr(), x.stride(0), stats.data_ptr(), x.shape[0], x.shape[1], float(eps),
                            1 if rms else 0, _dt(x), _stream())
    check(rc, "haff_row_stats")
    return stats


def linear_rowstats_supported(M, N, K, dtype, min_tiles=160):
    """Shapes whose residual product can emit the LayerNorm statistics of its output rows (haff_gemm_bf16_rowstats): whole
    256 x 256 tiles, and (min_tiles) enough of them that the 8-wave tile is what linear() would launch anyway."""
    return dtype in (torch.bfloat16, torch.float16) and M % 256 == 0 and N % 256 == 0 and K % 64 == 0 and (M // 256) * (N // 256) >= min_tiles


def rowstats_gemm(x, w, bias, resid, out, a_map=None):
    """The product of linear_rowstats alone (one haff_gemm_bf16_rowstats launch): returns the partial sums fp32 [M, N/64, 2]."""
    lib = load_library()
    M = a_map.numel() if a_map is not None else x.shape[0]
    N, K = w.shape
    part = torch.empty((M, N // 64, 2), dtype=torch.float32, device=x.device)
    rc = _fn(lib, "haff_gemm_bf16_rowstats", x.dtype)(x.data_ptr(), x.stride(0), _p(a_map), x.shape[0], w.data_ptr(), w.stride(0), out.data_ptr(),
                                     out.stride(0), _p(bias), resid.data_ptr(), resid.stride(0), M, N, K, part.data_ptr(), _stream())
    check(rc, "haff_gemm_bf16_rowstats")
    return part


def linear_rowstats(x, w, bias, resid, eps, out=None, a_map=None):
    """out = x @ w.T + bias + resid (bf16; out may be resid) AND the {mean, rstd} of every OUTPUT row as fp32 [M, 2] — the
    ln_stats of the next linear(..., ln_stats=): the producer's epilogue sums its own results, nobody reads the rows again."""
    lib = load_library()
    _req(x, "x")
    M, K = x.shape
    if a_map is not None:
        assert a_map.dtype == torch.int32
        M = a_map.numel()
    N = w.shape[0]
    assert x.dtype in (torch.bfloat16, torch.float16) and w.dtype == x.dtype and x.stride(1) == 1 and w.stride(1) == 1 and w.shape[1] == K
    assert linear_rowstats_supported(M, N, K, x.dtype, 0) and resid is not None and resid.dtype == x.dtype
    if out is None:
        out = torch.empty((M, N), dtype=x.dtype, device=x.device)
    part = rowstats_gemm(x, w, bias, resid, out, a_map)
    stats = torch.empty((M, 2), dtype=torch.float32, device=x.device)
    check(lib.haff_row_stats_finalize(part.data_ptr(), stats.data_ptr(), M, N // 64, N, float(eps), _stream()),
          "haff_row_stats_finalize")
    return out, stats


def rowstats32_gemm(x, w, bias, x32, out16, a_map=None):
    """The product of linear_rowstats32 alone (one haff_gemm_bf16_rowstats32 launch): returns the partial sums fp32 [M, N/64, 2]."""
    lib = load_library()
    M = a_map.numel() if a_map is not None else x.shape[0]
    N, K = w.shape
    part = torch.empty((M, N // 64, 2), dtype=torch.float32, device=x.device)
    rc = lib.haff_gemm_bf16_rowstats32(x.data_ptr(), x.stride(0), _p(a_map), x.shape[0], w.data_ptr(), w.stride(0), x32.data_ptr(),
                                       x32.stride(0), out16.data_ptr(), out16.stride(0), _p(bias), M, N, K, part.data_ptr(), _stream())
    check(rc, "haff_gemm_bf16_rowstats32")
    return part


def linear_rowstats32(x, w, bias, x32, out16, eps, a_map=None):
    """x32 += x @ w.T + bias IN PLACE on the fp32 residual stream, out16 = bf16(x32) (the next product's operand), and the
    {mean, rstd} of every row of the new x32 as fp32 [M, 2] (haff_gemm_bf16_rowstats32 + haff_row_stats_finalize)."""
    lib = load_library()
    _req(x, "x")
    M = a_map.numel() if a_map is not None else x.shape[0]
    N, K = w.shape
    assert x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and x.stride(1) == 1 and w.stride(1) == 1 and x.shape[1] == K
    assert x.dtype == torch.bfloat16 and x32.dtype == torch.float32 and out16.dtype == torch.bfloat16   # a bf16 epilogue
    assert linear_rowstats_supported(M, N, K, x.dtype, 0)
    assert x32.shape == (M, N) and out16.shape == (M, N) and x32.stride(1) == 1 and out16.stride(1) == 1 and bias is not None
    part = rowstats32_gemm(x, w, bias, x32, out16, a_map)
    stats = torch.empty((M, 2), dtype=torch.float32, device=x.device)
    check(lib.haff_row_stats_finalize(part.data_ptr(), stats.data_ptr(), M, N // 64, N, float(eps), _stream()),
          "haff_row_stats_finalize")
    return stats


def rope_permute_rows(w):
    """The row order haff_gemm_bf16_qkv_rope wants for the fused q|k|v weights [3*H*128, K]: inside every 256-row tile, natural
    row wn*64 + t*16 + i takes logical row (wn>>1)*128 + (t>>1)*64 + (wn&1)*32 + (t&1)*16 + i."""
    N = w.shape[0]
    assert N % 256 == 0
    j = torch.arange(256)
    wn, t, i = j // 64, (j // 16) % 4, j % 16
    logical = (wn // 2) * 128 + (t // 2) * 64 + (wn % 2) * 32 + (t % 2) * 16 + i
    idx = (torch.arange(0, N, 256)[:, None] + logical[None, :]).reshape(-1).to(w.device)
    return w.index_select(0, idx).contiguous()


def qkv_rope_supported(M, H, d, K, dtype, min_rows=1024):
    """Prefill-sized batches whose q|k|v projection can carry RoPE and the cache append (haff_gemm_bf16_qkv_rope): (min_rows)
    enough rows that the 8-wave tile is what linear() would launch anyway."""
    return dtype in (torch.bfloat16, torch.float16) and d == 128 and (H * d) % 256 == 0 and K % 64 == 0 and min_rows <= M < (1 << 22)


def qkv_rope(x, w_perm, kcache, vcache, cos_sin, B, T, H, d, pos0):
    """Rotated q [B*T, H*d] of x @ w.T; the rotated k and v rows land in kcache / vcache [B, Tmax, H*d] at pos0 .. pos0+T-1."""
    lib = load_library()
    _req(x, "x")
    M, K = x.shape
    assert M == B * T and w_perm.shape == (3 * H * d, K) and x.stride(1) == 1 and w_perm.stride(1) == 1
    assert x.dtype in (torch.bfloat16, torch.float16) and w_perm.dtype == x.dtype and kcache.dtype == x.dtype and vcache.dtype == x.dtype
    assert kcache.is_contiguous() and vcache.is_contiguous() and kcache.shape == vcache.shape and kcache.shape[2] == H * d
    assert cos_sin.dtype == torch.float32 and cos_sin.is_contiguous() and cos_sin.shape[0] >= kcache.shape[1] and cos_sin.shape[1] == d
    q = torch.empty((M, H * d), dtype=x.dtype, device=x.device)
    rc = _fn(lib, "haff_gemm_bf16_qkv_rope", x.dtype)(x.data_ptr(), x.stride(0), w_perm.data_ptr(), w_perm.stride(0), q.data_ptr(), q.stride(0),
                                     kcache.data_ptr(), vcache.data_ptr(), cos_sin.data_ptr(), B, T, kcache.shape[1], int(pos0),
                                     H, d, K, _stream())
    check(rc, "haff_gemm_bf16_qkv_rope")
    return q


def fold_norm(w, gamma, beta=None, bias=None, dtype=torch.bfloat16):
    """Fold y = norm(x) * gamma + beta followed by y @ w.T + bias into the weights: returns (w16 = dtype(w * gamma),
    colsum fp32 [N] of the ROUNDED folded weights, bias' = bias + w @ beta)."""
    wf = (w.float() * gamma.float()[None, :]).to(dtype).contiguous()
    colsum = wf.float().sum(1).contiguous()
    b = None
    if beta is not None or bias is not None:
        b = torch.zeros((w.shape[0],), dtype=torch.float32, device=w.device)
        if bias is not None:
            b += bias.float()
        if beta is not None:
            b += w.float() @ beta.float()
        b = b.contiguous()
    return wf, colsum, b


SPLIT_ROW_TAIL = True   # linear(): a <= 64-row tail that would cost the 8-wave tile an extra round goes out as its own launch


def linear(x, w, bias=None, act=ACT_NONE, resid=None, row_map=None, out=None, out_rows=None, out_dtype=None,
           swiglu=False, tile_cfg=0, a_map=None, ln_stats=None, ln_colsum=None):
    """y = epi(x @ w.T): x [M,K] (row stride free, unit inner stride), w [N,K], bias fp32 [N] or None.

    epilogue order: +bias -> act -> +resid (resid indexed like out). row_map (int32 [M]) redirects output
    (and residual) rows, negative entries are dropped. swiglu: w rows interleaved [gate x16 | up x16], N -> N/2.
    """
    lib = load_library()
    _req(x, "x")
    assert x.dim() == 2 and w.dim() == 2 and x.stride(1) == 1 and w.stride(1) == 1
    M, K = x.shape
    if a_map is not None:  # gather: logical row m reads x[a_map[m]] (bf16 only)
        assert a_map.dtype == torch.int32 and x.dtype in (torch.bfloat16, torch.float16)
        M = a_map.numel()
    N = w.shape[0]
    assert w.shape[1] == K, (x.shape, w.shape)
    out = _linear_out(x, M, N, swiglu, out, out_rows, out_dtype, resid, bias, row_map)
    if (SPLIT_ROW_TAIL and x.dtype in (torch.bfloat16, torch.float16) and M > 4096 and 0 < (M & 255) <= 64 and row_map is None and a_map is None
            and ln_stats is None and not swiglu and not tile_cfg and out_rows is None and N >= 256):
        # A short row tail that costs the persistent 256 x 256 tile a whole extra round (CLIP at 64 frames: 16448 rows = 64.25
        # row tiles; N = 1024 gives 260 tiles on 256 CUs, the last 4 alone in a second round: 758 TFLOP/s): the whole row
        # tiles and the <= 64 tail rows go out as two launches (the tail is a weight-streaming product)
        cols = (N + 255) // 256
        if -(-((M + 255) // 256 * cols) // 256) > -(-((M // 256) * cols) // 256):
            m0 = M & ~255
            _LINEAR(x[:m0], w, bias, act, None if resid is None else resid[:m0], out=out[:m0])
            _LINEAR(x[m0:], w, bias, act, None if resid is None else resid[m0:], out=out[m0:])
            return out
    xa, wc = (x.data_ptr(), x.stride(0)), (w.data_ptr(), w.stride(0), out.data_ptr(), out.stride(0))
    epi = _epilogue_args(out, bias, resid, row_map, M, N, K, act, swiglu)
    if ln_stats is not None:
        assert x.dtype in (torch.bfloat16, torch.float16) and w.dtype == x.dtype and a_map is None
        assert ln_stats.dtype == torch.float32 and ln_stats.shape == (M, 2) and ln_stats.is_contiguous()
        if ln_colsum is not None:
            assert ln_colsum.dtype == torch.float32 and ln_colsum.numel() == N
        rc = _fn(lib, "haff_gemm_bf16_ln", x.dtype)(*xa, *wc, *epi[:4], ln_stats.data_ptr(), _p(ln_colsum), *epi[4:], _stream())
    elif a_map is not None:
        assert w.dtype == x.dtype
        rc = _fn(lib, "haff_gemm_bf16_gather", x.dtype)(*xa, a_map.data_ptr(), x.shape[0], *wc, *epi, _stream())
    elif x.dtype in (torch.bfloat16, torch.float16) and 32 < M <= 1024 and not tile_cfg:
        # few output tiles (decode at batch 33..64 on narrow weights, prefill / CLIP at one frame): the library may split K
        # over workgroups through a per-stream fp32 workspace (partials summed in a fixed order)
        assert w.dtype == x.dtype
        ws = _workspace(x.device, 64 << 20)
        rc = _fn(lib, "haff_gemm_bf16_ws", x.dtype)(*xa, *wc, *epi, ws.data_ptr(), ws.numel(), _stream())
    elif x.dtype in (torch.bfloat16, torch.float16):
        assert w.dtype == x.dtype
        rc = _fn(lib, "haff_gemm_bf16_cfg", x.dtype)(*xa, *wc, *epi, tile_cfg, _stream())
    else:
        assert w.dtype == torch.float32 and out.dtype == torch.float32
        rc = lib.haff_gemm_f32(*xa, *wc, *epi[:8], epi[9], _stream())   # (fp32 out only: the signature has no out_f32)
    check(rc, "haff_gemm")
    return out


def nf4_quantize(w, double_quant=True, row_map=None, packed=None, absmax=None):
    """NF4 codes of an f16 weight [N, K] on the device (haff_nf4_quantize_f16; format: quant.py): returns (packed uint8 [R, K/2],
    dequantised absmax f32 [R, K/64], offset f32 [1]). row_map (int32 [N]): source row n goes to row row_map[n] of packed / absmax
    (given, with R rows; the q|k|v concatenation and the SwiGLU interleave); None: R = N, new tensors."""
    lib = load_library()
    _req(w, "w")
    assert w.dtype == torch.float16 and w.dim() == 2 and w.stride(1) == 1
    N, K = w.shape
    if K % 64:
        raise ValueError(f"NF4 needs K % 64 == 0 (K = {K})")
    if row_map is None:
        packed = torch.empty((N, K // 2), dtype=torch.uint8, device=w.device) if packed is None else packed
        absmax = torch.empty((N, K // 64), dtype=torch.float32, device=w.device) if absmax is None else absmax
        assert packed.shape[0] == N
    else:
        assert row_map.dtype == torch.int32 and row_map.numel() == N and packed is not None and absmax is not None
    assert packed.dtype == torch.uint8 and packed.is_contiguous() and packed.shape[1] == K // 2
    assert absmax.dtype == torch.float32 and absmax.is_contiguous() and absmax.shape == (packed.shape[0], K // 64)
    offset = torch.empty((1,), dtype=torch.float32, device=w.device)
    ws = torch.empty((N * (K // 64),), dtype=torch.float32, device=w.device)
    check(lib.haff_nf4_quantize_f16(w.data_ptr(), w.stride(0), N, K, 1 if double_quant else 0, _p(row_map), packed.data_ptr(),
                                    absmax.data_ptr(), offset.data_ptr(), ws.data_ptr(), ws.numel() * 4, _stream()),
          "haff_nf4_quantize_f16")
    return packed, absmax, offset


def _nf4_operands(packed, absmax):
    """(N, K) of an NF4 weight's stored rows: packed uint8 [N, K/2] and absmax f32 [N, K/64], both contiguous, in HBM"""
    _req(packed, "packed")
    N, K = packed.shape[0], packed.shape[1] * 2
    assert packed.dtype == torch.uint8 and packed.is_contiguous() and absmax.dtype == torch.float32 and absmax.is_contiguous()
    assert absmax.shape == (N, K // 64)
    return N, K


def nf4_dequant(packed, absmax, row_map=None, out=None):
    """f16 [N, K] = f16_rn(NF4[code] * absmax) of the stored rows; row_map (int32 [N]): stored row n goes to out row row_map[n]."""
    lib = load_library()
    N, K = _nf4_operands(packed, absmax)
    if out is None:
        out = torch.empty((N, K), dtype=torch.float16, device=packed.device)
    assert out.dtype == torch.float16 and out.stride(1) == 1 and out.shape[1] == K
    if row_map is not None:
        assert row_map.dtype == torch.int32 and row_map.numel() == N
    check(lib.haff_nf4_dequant_f16(packed.data_ptr(), absmax.data_ptr(), N, K, _p(row_map), out.data_ptr(), out.stride(0), _stream()),
          "haff_nf4_dequant_f16")
    return out


def _check_nf4_lora(lora, N, K):
    """The adapters of a fused NF4 weight [N, K] (quant.Nf4Lora): a_cat f16 [8 nseg, K], b f16 [N, 8], nseg, seg_rows, scale."""
    a, b = lora.a_cat, lora.b
    assert a.dtype == torch.float16 and a.dim() == 2 and a.stride(1) == 1 and a.shape == (8 * lora.nseg, K), (a.shape, lora.nseg, K)
    assert b.dtype == torch.float16 and b.is_contiguous() and b.shape == (N, 8), (b.shape, N)


def nf4_dequant_lora(packed, absmax, lora, row_map=None, out=None):
    """nf4_dequant with unmerged LoRA adapters folded in (haff_nf4_dequant_lora_f16): f16 [N, K] = f16_rn(NF4[code] * absmax +
    scale * (B A_cat)[n, k]), each stored row against its own segment's 8 rank rows of A_cat; same row_map contract."""
    lib = load_library()
    N, K = _nf4_operands(packed, absmax)
    _check_nf4_lora(lora, N, K)
    if out is None:
        out = torch.empty((N, K), dtype=torch.float16, device=packed.device)
    assert out.dtype == torch.float16 and out.stride(1) == 1 and out.shape[1] == K
    if row_map is not None:
        assert row_map.dtype == torch.int32 and row_map.numel() == N
    check(lib.haff_nf4_dequant_lora_f16(packed.data_ptr(), absmax.data_ptr(), N, K, _p(row_map), out.data_ptr(), out.stride(0),
                                        lora.a_cat.data_ptr(), lora.a_cat.stride(0), lora.b.data_ptr(), lora.nseg, lora.seg_rows,
                                        float(lora.scale), _stream()), "haff_nf4_dequant_lora_f16")
    return out


def nf4_dequant_t(packed, absmax, row_map=None, out=None):
    """f16 [K, Np] = the TRANSPOSE of nf4_dequant's result (stored row n in column row_map[n], or n), Np = roundup(N, 8), the pad
    columns zero: the layout autograd.transpose(w, Rp=_pad8(N)) gives a frozen weight's resident W^T (haff_nf4_dequant_t_f16).
    out: f16 [K, >= Np] with unit inner stride; its columns from Np on are left alone."""
    lib = load_library()
    N, K = _nf4_operands(packed, absmax)
    Np = (N + 7) // 8 * 8
    if out is None:
        out = torch.empty((K, Np), dtype=torch.float16, device=packed.device)
    assert out.dtype == torch.float16 and out.stride(1) == 1 and out.shape[0] == K and out.shape[1] >= Np
    if row_map is not None:
        assert row_map.dtype == torch.int32 and row_map.numel() == N
    check(lib.haff_nf4_dequant_t_f16(packed.data_ptr(), absmax.data_ptr(), N, K, _p(row_map), out.data_ptr(), out.stride(0), _stream()),
          "haff_nf4_dequant_t_f16")
    return out


def linear_nf4(x, packed, absmax, bias=None, act=ACT_NONE, resid=None, row_map=None, out=None, out_dtype=None, swiglu=False, lora=None,
               lora_t=None):
    """linear() with NF4 weights (haff_gemm_nf4_f16): x f16 [M <= 64, K], packed uint8 [N, K/2], absmax f32 [N, K/64]; same
    epilogue contract as linear(). lora (quant.Nf4Lora): the weight's unmerged adapters; scale * (x A_cat^T) B^T joins the fp32 sums
    before the epilogue (haff_gemm_nf4_lora_f16). lora_t: t = x A_cat^T as f16 [M, 8 nseg] when the caller has it (one
    linear(x, a_cat) launch otherwise)."""
    lib = load_library()
    _req(x, "x")
    assert x.dim() == 2 and x.stride(1) == 1 and x.dtype == torch.float16
    M, K = x.shape
    N = _nf4_operands(packed, absmax)[0]
    assert packed.shape[1] * 2 == K
    out = _linear_out(x, M, N, swiglu, out, None, out_dtype, resid, bias, row_map)
    assert out.dtype in (torch.float16, torch.float32)
    head = (x.data_ptr(), x.stride(0), packed.data_ptr(), absmax.data_ptr(), out.data_ptr(), out.stride(0))
    epi = _epilogue_args(out, bias, resid, row_map, M, N, K, act, swiglu)
    if lora is not None:
        _check_nf4_lora(lora, N, K)
        t = linear(x, lora.a_cat) if lora_t is None else lora_t
        assert t.dtype == torch.float16 and t.stride(1) == 1 and t.shape == (M, 8 * lora.nseg)
        rc = lib.haff_gemm_nf4_lora_f16(*head, *epi, t.data_ptr(), t.stride(0), lora.b.data_ptr(), lora.nseg, lora.seg_rows,
                                        float(lora.scale), _stream())
        check(rc, "haff_gemm_nf4_lora_f16")
        return out
    check(lib.haff_gemm_nf4_f16(*head, *epi, _stream()), "haff_gemm_nf4_f16")
    return out


def int8_quantize_weight(w, row_map=None, cb=None, scb=None):
    """LLM.int8 codes of an f16 weight [N, K] on the device (haff_int8_quantize_weight_f16; arithmetic: quant.py): returns
    (CB int8 [R, K], SCB f32 [R]). row_map (int32 [N]): source row n goes to row row_map[n] of the given cb / scb (R rows);
    None: R = N, new tensors unless given."""
    lib = load_library()
    _req(w, "w")
    assert w.dtype == torch.float16 and w.dim() == 2 and w.stride(1) == 1
    N, K = w.shape
    if K % 64:
        raise ValueError(f"int8 needs K % 64 == 0 (K = {K})")
    if cb is None:
        assert row_map is None
        cb = torch.empty((N, K), dtype=torch.int8, device=w.device)
        scb = torch.empty((N,), dtype=torch.float32, device=w.device)
    assert cb.dtype == torch.int8 and cb.is_contiguous() and cb.shape[1] == K
    assert scb.dtype == torch.float32 and scb.is_contiguous() and scb.numel() == cb.shape[0]
    if row_map is not None:
        assert row_map.dtype == torch.int32 and row_map.numel() == N
    else:
        assert cb.shape[0] == N
    check(lib.haff_int8_quantize_weight_f16(w.data_ptr(), w.stride(0), N, K, _p(row_map), cb.data_ptr(), scb.data_ptr(), _stream()),
          "haff_int8_quantize_weight_f16")
    return cb, scb


class Int8Rows:
    """The quantised activation rows of one int8 product: x (the f16 rows, for the outlier values), CA int8 [M, K], SCA f32 [M],
    cols int32 [S, K] / ncols int32 [S] (each segment's outlier columns, ascending), seg_rows."""

    def __init__(self, x, ca, sca, cols, ncols, seg_rows):
        self.x, self.ca, self.sca, self.cols, self.ncols, self.seg_rows = x, ca, sca, cols, ncols, seg_rows

def int8_quantize_act(x, threshold, seg_rows=None, valid=None, masks=None):
    """Row quantisation of f16 x [M, K] with the outlier decomposition (haff_int8_quantize_act_f16): segments of seg_rows rows (None:
    one segment), valid (int32 [S] device, or None: every row) = the rows of each segment whose outliers count, masks (uint32-as-int32
    [S, K/32] device; ORed into, so pass zeros for a fresh call or a frame's sticky masks; None: a zeroed scratch). -> Int8Rows."""
    lib = load_library()
    _req(x, "x")
    assert x.dtype == torch.float16 and x.dim() == 2 and x.stride(1) == 1
    M, K = x.shape
    seg_rows = M if seg_rows is None else int(seg_rows)
    S = (M + seg_rows - 1) // seg_rows
    if K % 64:
        raise ValueError(f"int8 needs K % 64 == 0 (K = {K})")
    if threshold < 0:
        raise ValueError(f"llm_int8_threshold must be >= 0 (got {threshold})")
    dev = x.device
    if masks is None and threshold > 0:
        masks = torch.zeros((S, K // 32), dtype=torch.int32, device=dev)
    if masks is not None:
        assert masks.dtype == torch.int32 and masks.is_contiguous() and masks.shape == (S, K // 32)
    if valid is not None:
        assert valid.dtype == torch.int32 and valid.numel() == S
    ca = torch.empty((M, K), dtype=torch.int8, device=dev)
    sca = torch.empty((M,), dtype=torch.float32, device=dev)
    cols = torch.empty((S, K), dtype=torch.int32, device=dev)
    ncols = torch.empty((S,), dtype=torch.int32, device=dev)
    check(lib.haff_int8_quantize_act_f16(x.data_ptr(), x.stride(0), M, K, float(threshold), seg_rows, _p(valid), _p(masks),
                                         ca.data_ptr(), K, sca.data_ptr(), cols.data_ptr(), ncols.data_ptr(), _stream()),
          "haff_int8_quantize_act_f16")
    return Int8Rows(x, ca, sca, cols, ncols, seg_rows)


INT8_AUTO, INT8_SKINNY, INT8_TILED = 0, 1, 2


def linear_int8(q, cb, scb, bias=None, act=ACT_NONE, resid=None, row_map=None, out=None, out_dtype=None, swiglu=False, form=INT8_AUTO):
    """linear() with LLM.int8 weights (haff_gemm_int8_f16): q = int8_quantize_act(...) of the input rows, cb int8 [N, K], scb f32 [N];
    same epilogue contract as linear(), applied to the f16 product Y. form: INT8_AUTO (by M), INT8_SKINNY (M <= 64), INT8_TILED."""
    lib = load_library()
    x = q.x
    M, K = x.shape
    N = cb.shape[0]
    assert cb.dtype == torch.int8 and cb.is_contiguous() and cb.shape[1] == K and scb.numel() == N
    out = _linear_out(x, M, N, swiglu, out, None, out_dtype, resid, bias, row_map)
    assert out.dtype in (torch.float16, torch.float32)
    rc = lib.haff_gemm_int8_f16(x.data_ptr(), x.stride(0), q.ca.data_ptr(), q.ca.stride(0), q.sca.data_ptr(), cb.data_ptr(),
                                scb.data_ptr(), q.cols.data_ptr(), q.ncols.data_ptr(), q.seg_rows, out.data_ptr(), out.stride(0),
                                *_epilogue_args(out, bias, resid, row_map, M, N, K, act, swiglu), int(form), _stream())
    check(rc, "haff_gemm_int8_f16")
    return out


def linear_heads_supported(M, N, K, d, heads, dtype):
    """Shapes haff_gemm_bf16_heads serves: whole 256 x 256 tiles of the 8-wave kernel, N = parts * heads * d."""
    return (dtype in (torch.bfloat16, torch.float16) and M % 256 == 0 and N % 256 == 0 and K % 64 == 0 and d % 8 == 0 and N % (heads * d) == 0
            and N // (heads * d) <= 3 and heads * d < (1 << 16) and M * K * 2 < (1 << 32) and N * K * 2 < (1 << 32))


def gemm_stream_cap(cap, stream=None):
    """Workgroups per launch of the persistent GEMM tile for launches enqueued on `stream` (a torch stream; default: the current
    one) from now on (haff_gemm_stream_cap; 256 = every CU). Returns the stream's previous setting. Scheduling only: outputs do
    not depend on it, launches on other streams are unaffected."""
    s = _stream() if stream is None else stream.cuda_stream
    rc = int(load_library().haff_gemm_stream_cap(s, int(cap)))
    if rc < 0:
        check(rc, "haff_gemm_stream_cap")
    return rc


def linear_heads(x, w, bias, row_map, out, d, heads, part_stride, head_stride, ln_stats=None, ln_colsum=None):
    """x @ w.T (+ folded norm) scattered HEAD-MAJOR into `out` (haff_gemm_bf16_heads): product column part * heads * d + h * d + c of
    row m goes to out.flat[part * part_stride + h * head_stride + row_map[m] * d + c]."""
    lib = load_library()
    _req(x, "x")
    M, K = x.shape
    N = w.shape[0]
    assert x.dtype in (torch.bfloat16, torch.float16) and w.dtype == x.dtype and out.dtype == x.dtype and out.is_contiguous()
    assert x.stride(1) == 1 and w.stride(1) == 1 and w.shape[1] == K and row_map.dtype == torch.int32 and row_map.numel() == M
    assert bias is None or (bias.dtype == torch.float32 and bias.numel() == N)
    if ln_stats is not None:
        assert ln_stats.dtype == torch.float32 and ln_stats.shape == (M, 2) and ln_stats.is_contiguous()
    parts = N // (heads * d)
    assert out.numel() >= (parts - 1) * part_stride + heads * head_stride   # (the row map's range is the caller's contract)
    rc = _fn(lib, "haff_gemm_bf16_heads", x.dtype)(x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), out.data_ptr(), _p(bias), row_map.data_ptr(),
                                  _p(ln_stats), _p(ln_colsum), M, N, K, d, heads, part_stride, head_stride, _stream())
    check(rc, "haff_gemm_bf16_heads")
    return out


_LINEAR = linear   # the function itself: linear()'s own two-launch form must not go through a wrapper installed on ops.linear (bench.py's meter)


def _half(t):
    return t.dtype in (torch.bfloat16, torch.float16)


def linear_rms(x, w, resid=None, out=None, swiglu=False, ssq_in=None, ssq_out=None, eps=0.0):
    """Decode-sized bf16 product (M <= 16) carrying RMSNorm statistics between products (haff_gemm_bf16_rms):
    ssq_in fp32 [parts,16]: rows are scaled by rsqrt(sum(ssq_in[:, m]) / K + eps) (w = gamma-folded weights, x = raw
    residual stream); ssq_out fp32 [>= N/16, 16]: receives this product's per-workgroup sums of squares of the bf16 output."""
    lib = load_library()
    _req(x, "x")
    M, K = x.shape
    N = w.shape[0]
    assert x.dtype in (torch.bfloat16, torch.float16) and w.dtype == x.dtype and x.stride(1) == 1 and w.stride(1) == 1 and w.shape[1] == K
    out = _linear_out(x, M, N, swiglu, out, None, None, resid, None, None)
    assert out.dtype == x.dtype and out.shape[0] == M
    if ssq_in is not None:
        assert ssq_in.dtype == torch.float32 and ssq_in.is_contiguous() and ssq_in.shape[1] == 16
    if ssq_out is not None:
        assert ssq_out.dtype == torch.float32 and ssq_out.is_contiguous() and ssq_out.shape[1] == 16 and ssq_out.shape[0] * 16 >= N
    rc = _fn(lib, "haff_gemm_bf16_rms", x.dtype)(x.data_ptr(), x.stride(0), w.data_ptr(), w.stride(0), out.data_ptr(), out.stride(0), None,
                                _p(resid), 0 if resid is None else resid.stride(0), M, N, K, ACT_NONE, 0, 1 if swiglu else 0,
                                _p(ssq_in), 0 if ssq_in is None else ssq_in.shape[0], float(eps), _p(ssq_out), None, _stream())
    check(rc, "haff_gemm_bf16_rms")
    return out


class ChainLayer(ctypes.Structure):
    """haff_chain_layer of include/haff_hip.h: the six device pointers of one Llama layer on the chained decode step."""
    _fields_ = [(n, ctypes.c_void_p) for n in ("wqkv", "wo", "wgu", "wd", "kcache", "vcache")]


def decode_chain_supported(M, hidden, ffn, heads, n_layers):
    return int(load_library().haff_decode_chain_supported(int(M), int(hidden), int(ffn), int(heads), int(n_layers))) > 0


def decode_chain_sync_words(n_layers, hidden):
    return int(load_library().haff_decode_chain_sync_words(int(n_layers), int(hidden)))


def decode_chain_table(layers):
    """layers: one (wqkv, wo, wgu, wd, kcache, vcache) tuple of bf16 tensors per layer -> the host table haff_decode_chain_bf16 takes."""
    for row in layers:
        for t in row:
            _req(t, "chain operand")
            assert t.dtype == torch.bfloat16 and t.is_contiguous()
    return (ChainLayer * len(layers))(*[ChainLayer(*[t.data_ptr() for t in row]) for row in layers])


def decode_chain(table, n_layers, x, qkv, att, g, ssq_a, ssq_b, ws, stats0, eps, cos_sin, nk_rows, heads, tmax, scale, sync,
                 per_stage_launches=False):
    """One KV-cached decode step of the whole Llama stack at <= 8 rows as ONE launch (haff_decode_chain_bf16): x [M,H] bf16 is
    the residual stream (in place); qkv [M,3H], att [M,H], g [M,F], ssq_a / ssq_b f32 [H/16,16]: scratch; stats0 f32 [M,2];
    ws f32 [H/16, 2, 16, 16]: scratch; sync uint32 (int32 tensor) [decode_chain_sync_words(n_layers, H)], zeroed once at allocation. per_stage_launches: the same kernel, one launch per
    (layer, stage) — identical arithmetic without the chaining (tests, A/B)."""
    lib = load_library()
    _req(x, "x")
    M, H = x.shape
    F = g.shape[1]
    assert x.dtype == torch.bfloat16 and x.is_contiguous() and qkv.is_contiguous() and att.is_contiguous() and g.is_contiguous()
    assert qkv.shape == (M, 3 * H) and att.shape == (M, H) and g.shape[0] == M
    assert ssq_a.dtype == torch.float32 and ssq_a.shape == (H // 16, 16) and ssq_b.shape == (H // 16, 16)
    assert stats0.dtype == torch.float32 and stats0.shape == (M, 2) and stats0.is_contiguous()
    assert nk_rows.dtype == torch.int32 and nk_rows.numel() == M and cos_sin.dtype == torch.float32 and cos_sin.shape[1] == 128
    assert sync.dtype == torch.int32 and sync.numel() >= decode_chain_sync_words(n_layers, H)
    assert ws.dtype == torch.float32 and ws.is_contiguous() and ws.numel() >= (H // 16) * 2 * 256
    rc = lib.haff_decode_chain_bf16(table, int(n_layers), M, H, F, int(heads), x.data_ptr(), qkv.data_ptr(), att.data_ptr(),
                                    g.data_ptr(), ssq_a.data_ptr(), ssq_b.data_ptr(), ws.data_ptr(), stats0.data_ptr(), float(eps),
                                    cos_sin.data_ptr(), nk_rows.data_ptr(), int(tmax), float(scale), sync.data_ptr(),
                                    1 if per_stage_launches else 0, _stream())
    check(rc, "haff_decode_chain_bf16")
    return x


def decode_chain_status(sync, n_layers):
    """True when every bounded wait of the chained launches so far was satisfied (synchronises the current stream)."""
    rc = int(load_library().haff_decode_chain_status(sync.data_ptr(), int(n_layers), _stream()))
    if rc < 0:
        check(rc, "haff_decode_chain_status")
    return rc == 0


def _qkvo(q, k, v, out):
    """The 16 operand arguments the attention entry points start with — base address and (batch, head, token) strides of the q, k, v
    [B,H,N,d] views and of the token-major output [B,Nq,H*d] seen the same way — and that output, allocated here when out is None."""
    B, H, Nq, d = q.shape
    if out is None:
        out = torch.empty((B, Nq, H * d), dtype=q.dtype, device=q.device)
    (q_sb, q_sh, q_st, _), (k_sb, k_sh, k_st, _), (v_sb, v_sh, v_st, _) = q.stride(), k.stride(), v.stride()
    o_sb, o_st, o_sh, _ = out.view(B, Nq, H, d).stride()
    return [q.data_ptr(), q_sb, q_sh, q_st, k.data_ptr(), k_sb, k_sh, k_st, v.data_ptr(), v_sb, v_sh, v_st,
            out.data_ptr(), o_sb, o_sh, o_st], out


def attention(q, k, v, scale, causal=False, q_pos0=0, relh=None, relw=None, S=0, out=None):
    """q [B,H,Nq,d], k/v [B,H,Nk,d] strided views (unit stride on d). Returns out [B,Nq,H*d] (token-major)."""
    lib = load_library()
    _req(q, "q")
    B, H, Nq, d = q.shape
    Nk = k.shape[2]
    assert q.stride(3) == 1 and k.stride(3) == 1 and v.stride(3) == 1
    qkvo, out = _qkvo(q, k, v, out)
    if relh is not None:
        assert relh.dtype == torch.float32 and relh.is_contiguous() and relw.is_contiguous()
    rc = _fn(lib, "haff_attention_bf16", q.dtype, f32=True)(*qkvo, B, H, Nq, Nk, d, float(scale), 1 if causal else 0, int(q_pos0),
                                                            _p(relh), _p(relw), int(S), _stream())
    check(rc, "haff_attention")
    return out


_BF16_TABLES = {}


def _bf16_table(t, dtype=torch.bfloat16):
    """t rounded to the 16-bit format of the fused rel-pos kernels (bf16, or fp16 in the fp16 mode), once per tensor."""
    key = (t.data_ptr(), tuple(t.shape), dtype)
    hit = _BF16_TABLES.get(key)
    if hit is None or hit[0] is not t:
        _BF16_TABLES[key] = (t, t.to(dtype).contiguous())
    return _BF16_TABLES[key][1]


def relpos_tables(q, tab_h, tab_w, S):
    """q [B,H,N,d] view with N == S*S; tab_* fp32 [2S-1,d]. Returns relh, relw fp32 [B*H,N,S]."""
    lib = load_library()
    B, H, N, d = q.shape
    assert N == S * S and tab_h.shape == (2 * S - 1, d) and tab_h.dtype == torch.float32
    relh = torch.empty((B * H, N, S), dtype=torch.float32, device=q.device)
    relw = torch.empty_like(relh)
    if q.dtype == torch.bfloat16:
        # throughput mode: MFMA kernel on bf16 tables (the reference's bf16 checkpoint stores them in bf16 too)
        th, tw = _bf16_table(tab_h), _bf16_table(tab_w)
        rc = lib.haff_relpos_tables_bf16(q.data_ptr(), q.stride(0), q.stride(1), q.stride(2), th.data_ptr(),
                                         tw.data_ptr(), relh.data_ptr(), relw.data_ptr(), B, H, S, d, _stream())
        check(rc, "haff_relpos_tables_bf16")
        return relh, relw
    rc = lib.haff_relpos_tables(q.data_ptr(), q.stride(0), q.stride(1), q.stride(2), tab_h.data_ptr(),
                                tab_w.data_ptr(), relh.data_ptr(), relw.data_ptr(), B, H, S, d, _dt(q), _stream())
    check(rc, "haff_relpos_tables")
    return relh, relw


def window_attention_supported(q, S):
    """Geometry served by the fused window kernel (haff_window_attention_bf16)."""
    return q.dtype in (torch.bfloat16, torch.float16) and S == 14 and q.shape[3] == 80 and q.shape[2] == S * S


def window_attention(q, k, v, scale, tab_h, tab_w, S, out=None, grid=0, pad_token=0):
    """Fused SAM window attention + decomposed rel-pos. q/k/v [n_windows,H,S*S,d] strided views, tab_* fp32 [2S-1,d]
    (rounded to bf16 once and cached, as the reference's bf16 checkpoint stores them). Returns [n_windows,S*S,H*d].
    grid > 0: windows tile grid x grid token images and the padded window tokens were never written; their q/k/v
    are taken from token row `pad_token` of the views (the caller stores the qkv bias there)."""
    lib = load_library()
    _req(q, "q")
    B, H, _, d = q.shape
    assert window_attention_supported(q, S) and q.stride(3) == 1 and k.stride(3) == 1 and v.stride(3) == 1
    th, tw = _bf16_table(tab_h, q.dtype), _bf16_table(tab_w, q.dtype)
    qkvo, out = _qkvo(q, k, v, out)
    rc = _fn(lib, "haff_window_attention_bf16", q.dtype)(*qkvo, B, H, S, d, float(scale), th.data_ptr(), tw.data_ptr(), int(grid),
                                                         int(grid), int(pad_token), _stream())
    check(rc, "haff_window_attention_bf16")
    return out


def global_attention_supported(q, k, v, S):
    """Geometry served by the fused global kernel (haff_global_attention_bf16): ViT-H global blocks, k|v in one row layout."""
    return (q.dtype in (torch.bfloat16, torch.float16) and S == 64 and q.shape[3] == 80 and q.shape[2] == S * S and k.shape[2] == S * S
            and k.stride() == v.stride() and v.data_ptr() >= k.data_ptr()
            and (v.data_ptr() - k.data_ptr()) + k.shape[2] * k.stride(2) * 2 < (1 << 31))


def global_attention(q, k, v, scale, tab_h, tab_w, S, out=None):
    """Fused SAM global attention + decomposed rel-pos (no rel-pos tables in HBM). q/k/v [B,H,S*S,d] strided views, tab_* fp32
    [2S-1,d] (rounded to bf16 once and cached, as the reference's bf16 checkpoint stores them). Returns [B,S*S,H*d]."""
    lib = load_library()
    _req(q, "q")
    B, H, _, d = q.shape
    assert global_attention_supported(q, k, v, S) and q.stride(3) == 1 and k.stride(3) == 1 and v.stride(3) == 1
    th, tw = _bf16_table(tab_h, q.dtype), _bf16_table(tab_w, q.dtype)
    qkvo, out = _qkvo(q, k, v, out)
    rc = _fn(lib, "haff_global_attention_bf16", q.dtype)(*qkvo, B, H, S, d, float(scale), th.data_ptr(), tw.data_ptr(), _stream())
    check(rc, "haff_global_attention_bf16")
    return out


def _norm_dt(x, out):
    """dtype code of the norm kernels: 0 bf16, 1 f32, 3 f16, 2 = f32 rows in, bf16 rows out (fp32 residual stream -> bf16 product)."""
    if x.dtype == torch.float32 and out.dtype == torch.bfloat16:
        return 2
    assert out.dtype == x.dtype, (x.dtype, out.dtype)
    return _dt(x)


def layernorm(x, w, b, eps, in_map=None, out=None, out_dtype=None):
    """x [R,C]; optional gather map (int32 [R_out], <0 -> zero row). out_dtype=torch.bfloat16 on fp32 rows: one rounding, of the
    normalised row."""
    lib = load_library()
    _req(x, "x")
    assert x.dim() == 2 and x.stride(1) == 1
    rows = x.shape[0] if in_map is None else in_map.numel()
    C = x.shape[1]
    if out is None:
        out = torch.empty((rows, C), dtype=out_dtype or x.dtype, device=x.device)
    rc = lib.haff_layernorm(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), w.data_ptr(), b.data_ptr(),
                            _p(in_map), rows, C, float(eps), _norm_dt(x, out), _stream())
    check(rc, "haff_layernorm")
    return out


def rmsnorm(x, w, eps, out=None, out_dtype=None):
    lib = load_library()
    _req(x, "x")
    assert x.dim() == 2 and x.stride(1) == 1
    if out is None:
        out = torch.empty(x.shape, dtype=out_dtype or x.dtype, device=x.device)
    rc = lib.haff_rmsnorm(x.data_ptr(), x.stride(0), out.data_ptr(), out.stride(0), w.data_ptr(), x.shape[0],
                          x.shape[1], float(eps), _norm_dt(x, out), _stream())
    check(rc, "haff_rmsnorm")
    return out


def patchify_nchw(x, P, gh, gw, Kp, out_dtype):
    lib = load_library()
    _req(x, "x")
    x = x.contiguous()
    B, Cin, Hin, Win = x.shape
    out = torch.empty((B * gh * gw, Kp), dtype=out_dtype, device=x.device)
    rc = lib.haff_patchify_nchw(x.data_ptr(), out.data_ptr(), B, Cin, Hin, Win, P, gh, gw, Kp, _dt(x), _dt(out),
                                _stream())
    check(rc, "haff_patchify_nchw")
    return out


def patchify_u8(frames, P, gh, gw, Kp, mean3, std3, out_dtype):
    """frames uint8 NHWC [B,Hf,Wf,3]; mean3/std3 host sequences of 3 floats (0..255 scale)."""
    lib = load_library()
    _req(frames, "frames")
    assert frames.dtype == torch.uint8 and frames.is_contiguous() and frames.shape[3] == 3
    B, Hf, Wf, _ = frames.shape
    out = torch.empty((B * gh * gw, Kp), dtype=out_dtype, device=frames.device)
    m = (ctypes.c_float * 3)(*[float(v) for v in mean3])
    s = (ctypes.c_float * 3)(*[float(v) for v in std3])
    rc = lib.haff_patchify_u8(frames.data_ptr(), out.data_ptr(), B, Hf, Wf, P, gh, gw, Kp,
                              ctypes.cast(m, ctypes.c_void_p), ctypes.cast(s, ctypes.c_void_p), _dt(out), _stream())
    check(rc, "haff_patchify_u8")
    return out


def im2col3x3(x):
    """x [B,H,W,C] channels-last contiguous -> [B*H*W, 9*C]."""
    lib = load_library()
    _req(x, "x")
    assert x.is_contiguous()
    B, H, W, C = x.shape
    out = torch.empty((B * H * W, 9 * C), dtype=x.dtype, device=x.device)
    rc = lib.haff_im2col3x3(x.data_ptr(), out.data_ptr(), B, H, W, C, _dt(x), _stream())
    check(rc, "haff_im2col3x3")
    return out


def embed_splice(ids, img_pos, embed, img):
    """ids int64 [B,L] (sentinel < 0 at img_pos[b]); embed [V,Hd]; img [B,n_img,Hd] -> [B, L+n_img-1, Hd]."""
    lib = load_library()
    _req(ids, "ids")
    B, L = ids.shape
    n_img, Hd = img.shape[1], img.shape[2]
    assert ids.dtype == torch.int64 and ids.is_contiguous() and img.is_contiguous() and embed.is_contiguous()
    assert img_pos.dtype == torch.int32
    out = torch.empty((B, L + n_img - 1, Hd), dtype=embed.dtype, device=embed.device)
    rc = lib.haff_embed_splice(ids.data_ptr(), img_pos.data_ptr(), embed.data_ptr(), img.data_ptr(), out.data_ptr(),
                               B, L, n_img, Hd, _dt(embed), _stream())
    check(rc, "haff_embed_splice")
    return out


def rope_cache(qkv, kcache, vcache, cos_sin, B, Tq, Hq, Hkv, d, pos0):
    """qkv [B*Tq, (Hq+2Hkv)*d] rotated in place; k,v appended to caches [B,Tmax,Hkv*d]."""
    lib = load_library()
    _req(qkv, "qkv")
    Tmax = kcache.shape[1]
    assert kcache.is_contiguous() and vcache.is_contiguous() and cos_sin.dtype == torch.float32
    rc = lib.haff_rope_cache(qkv.data_ptr(), qkv.stride(0), kcache.data_ptr(), vcache.data_ptr(), cos_sin.data_ptr(),
                             B, Tq, Hq, Hkv, d, pos0, Tmax, _dt(qkv), _stream())
    check(rc, "haff_rope_cache")


def rope_cache_rows(qkv, kcache, vcache, cos_sin, B, Tq, Hq, Hkv, d, pos0_rows):
    """rope_cache with a per-row start position (int32 [B] on the device): ragged right-padded batches."""
    lib = load_library()
    _req(qkv, "qkv")
    Tmax = kcache.shape[1]
    assert kcache.is_contiguous() and vcache.is_contiguous() and cos_sin.dtype == torch.float32
    assert pos0_rows.dtype == torch.int32 and pos0_rows.is_cuda and pos0_rows.numel() == B
    rc = lib.haff_rope_cache_rows(qkv.data_ptr(), qkv.stride(0), kcache.data_ptr(), vcache.data_ptr(), cos_sin.data_ptr(),
                                  B, Tq, Hq, Hkv, d, pos0_rows.data_ptr(), Tmax, _dt(qkv), _stream())
    check(rc, "haff_rope_cache_rows")


def kv_prefix_broadcast(k_src, v_src, k_dst, v_dst, frame_of, P):
    """Positions 0 .. P-1 of the K and V caches k_src / v_src [F,tmax_src,H], row frame_of[b], into row b of k_dst / v_dst
    [B,tmax_dst,H] (haff_kv_prefix_broadcast: one launch for both tensors). frame_of int32 [B] on the device, every entry in [0, F):
    the caller has validated it (prompt_groups.check_offset); positions >= P of the destination keep their bytes."""
    lib = load_library()
    _req(k_src, "k_src")
    F, _, H = k_src.shape
    B = k_dst.shape[0]
    for s, d in ((k_src, k_dst), (v_src, v_dst)):
        assert s.dim() == 3 and d.dim() == 3 and s.shape == k_src.shape and d.shape == k_dst.shape and d.shape[2] == H
        assert s.dtype == k_src.dtype and d.dtype == k_src.dtype and s.stride() == k_src.stride() and d.stride() == k_dst.stride()
        assert s.stride(2) == 1 and d.stride(2) == 1 and s.stride(1) == H and d.stride(1) == H
    assert 1 <= P <= k_src.shape[1] and P <= k_dst.shape[1], (P, k_src.shape, k_dst.shape)
    assert frame_of.dtype == torch.int32 and frame_of.is_cuda and frame_of.is_contiguous() and frame_of.numel() == B
    rc = lib.haff_kv_prefix_broadcast(k_src.data_ptr(), v_src.data_ptr(), k_src.stride(0), k_dst.data_ptr(), v_dst.data_ptr(),
                                      k_dst.stride(0), frame_of.data_ptr(), B, F, int(P), H, _dt(k_src), _stream())
    check(rc, "haff_kv_prefix_broadcast")


def attention_decode_rows(q, k, v, scale, nk_rows, out=None):
    """One query per (batch, head) against ragged KV caches: q [B,H,1,d] view, k/v [B,H,Nk,d] views of the whole cache,
    nk_rows int32 [B] on the device (keys visible per batch entry). Returns [B,1,H*d]."""
    lib = load_library()
    _req(q, "q")
    B, H, Nq, d = q.shape
    assert Nq == 1 and q.stride(3) == 1 and k.stride(3) == 1 and v.stride(3) == 1
    assert nk_rows.dtype == torch.int32 and nk_rows.is_cuda and nk_rows.numel() == B
    qkvo, out = _qkvo(q, k, v, out)
    del qkvo[15], qkvo[3]   # one query row per (batch, head): the entry point takes no token stride for q and the output
    rc = _fn(lib, "haff_attention_decode_rows_bf16", q.dtype, f32=True)(*qkvo, B, H, k.shape[2], d, float(scale), nk_rows.data_ptr(),
                                                                        _stream())
    check(rc, "haff_attention_decode_rows")
    return out


def decode_attention_rope(qkv, kcache, vcache, cos_sin, H, d, scale, nk_rows):
    """bf16 / fp16 decode position with RoPE + cache append fused: qkv [B, 3*H*d] raw -> [B, 1, H*d]; nk_rows int32 [B] = new pos + 1."""
    lib = load_library()
    _req(qkv, "qkv")
    B = qkv.shape[0]
    assert _half(qkv) and qkv.stride(1) == 1 and kcache.is_contiguous() and vcache.is_contiguous()
    assert kcache.dtype == qkv.dtype and vcache.dtype == qkv.dtype
    assert nk_rows.dtype == torch.int32 and nk_rows.is_cuda and nk_rows.numel() == B and cos_sin.dtype == torch.float32
    out = torch.empty((B, 1, H * d), dtype=qkv.dtype, device=qkv.device)
    rc = _fn(lib, "haff_decode_attention_rope_rows_bf16", qkv.dtype)(qkv.data_ptr(), qkv.stride(0), kcache.data_ptr(), vcache.data_ptr(),
                                                                     cos_sin.data_ptr(), out.data_ptr(), B, H, d, kcache.shape[1],
                                                                     float(scale), nk_rows.data_ptr(), _stream())
    check(rc, "haff_decode_attention_rope_rows")
    return out


def argmax_rows(logits):
    lib = load_library()
    _req(logits, "logits")
    assert logits.dtype == torch.float32 and logits.stride(1) == 1
    out = torch.empty((logits.shape[0],), dtype=torch.int64, device=logits.device)
    rc = lib.haff_argmax_rows(logits.data_ptr(), logits.stride(0), out.data_ptr(), logits.shape[0], logits.shape[1],
                              _stream())
    check(rc, "haff_argmax_rows")
    return out


def decode_book(nxt_raw, st, h1, pad, eos):
    """Device-side bookkeeping of one greedy-decode token (haff_decode_book). st: the persistent per-(batch, capacity) state
    dict of LisaMI355._persistent_cache (forced, use_forced, steps, finished, out_ids, lens, t_rows, tok, pos, nk, hidden)."""
    lib = load_library()
    _req(nxt_raw, "nxt_raw")
    B = nxt_raw.shape[0]
    hid = st["hidden"]
    assert nxt_raw.dtype == torch.int64 and st["out_ids"].dtype == torch.int64 and st["forced"].dtype == torch.int64
    assert hid.is_contiguous() and (h1 is None or (h1.is_contiguous() and h1.numel() == B * hid.shape[2] and h1.dtype == hid.dtype))
    rc = lib.haff_decode_book(nxt_raw.data_ptr(), st["forced"].data_ptr(), st["forced"].stride(0), st["use_forced"].data_ptr(),
                              st["steps"].data_ptr(), st["finished"].data_ptr(), st["out_ids"].data_ptr(), st["out_ids"].stride(0),
                              st["lens"].data_ptr(), st["t_rows"].data_ptr(), st["tok"].data_ptr(), st["pos"].data_ptr(),
                              st["nk"].data_ptr(), _p(h1), hid.data_ptr(), hid.stride(0) * hid.element_size(),
                              hid.shape[2] * hid.element_size(), int(pad), int(eos), B, _stream())
    check(rc, "haff_decode_book")


def add_bcast(a, b, mod=None, out=None):
    """out[r] = a[r] + b[r % mod]; a [R,C], b [mod,C]."""
    lib = load_library()
    _req(a, "a")
    assert a.is_contiguous() and b.is_contiguous() and a.dtype == b.dtype
    R, C = a.shape
    mod = b.shape[0] if mod is None else mod
    if out is None:
        out = torch.empty_like(a)
    rc = lib.haff_add_bcast(a.data_ptr(), b.data_ptr(), out.data_ptr(), R, C, mod, _dt(a), _stream())
    check(rc, "haff_add_bcast")
    return out


def softmax_rows(x):
    lib = load_library()
    _req(x, "x")
    assert x.is_contiguous() and x.dim() == 2
    out = torch.empty(x.shape, dtype=torch.float32, device=x.device)
    rc = lib.haff_softmax_rows(x.data_ptr(), out.data_ptr(), x.shape[0], x.shape[1], _dt(x), _stream())
    check(rc, "haff_softmax_rows")
    return out


def upscale_mask(up1, ln_w, ln_b, w2, b2, hyper, n_prompts, h, w, eps=1e-6):
    lib = load_library()
    _req(up1, "up1")
    assert up1.is_contiguous() and up1.shape == (n_prompts * h * w, 256)
    assert hyper.dtype == torch.float32 and hyper.is_contiguous() and hyper.shape == (n_prompts, 32)
    out = torch.empty((n_prompts, 4 * h, 4 * w), dtype=torch.float32, device=up1.device)
    rc = lib.haff_upscale_mask(up1.data_ptr(), ln_w.data_ptr(), ln_b.data_ptr(), w2.data_ptr(), b2.data_ptr(),
                               hyper.data_ptr(), out.data_ptr(), n_prompts, h, w, float(eps), _dt(up1), _stream())
    check(rc, "haff_upscale_mask")
    return out


def resize_bilinear(x, crop_hw, out_hw):
    """x fp32 [N,Hs,Ws]; resample its top-left crop to out_hw (F.interpolate bilinear, align_corners=False)."""
    lib = load_library()
    _req(x, "x")
    assert x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 3
    N, Hs, Ws = x.shape
    out = torch.empty((N, out_hw[0], out_hw[1]), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.haff_resize_bilinear(x.data_ptr(), out.data_ptr(), N, Hs, Ws, int(crop_hw[0]), int(crop_hw[1]),
                                      int(out_hw[0]), int(out_hw[1]), _stream())
    check(rc, "haff_resize_bilinear")
    return out


def threshold_masks(x, logit_th=0.0):
    lib = load_library()
    _req(x, "x")
    assert x.dtype == torch.float32 and x.is_contiguous()
    out = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    with torch.cuda.device(x.device):
        rc = lib.haff_threshold_masks(x.data_ptr(), out.data_ptr(), x.numel(), float(logit_th), _stream())
    check(rc, "haff_threshold_masks")
    return out


def gate_threshold_masks(x, logit_ths, on_value=255, taxonomy=None, blank_class=-1):
    """x fp32 [...] mask logits of ONE prompt -> uint8 [n_th, ...]: (argmax(taxonomy) != blank_class and x > th) ? on_value : 0."""
    lib = load_library()
    _req(x, "x")
    assert x.dtype == torch.float32 and x.is_contiguous()
    n_th = len(logit_ths)
    total = x.numel()
    stride = (total + 3) // 4 * 4
    buf = torch.empty((n_th, stride), dtype=torch.uint8, device=x.device)
    ths = (ctypes.c_float * n_th)(*[float(v) for v in logit_ths])
    if taxonomy is not None:
        assert taxonomy.dtype == torch.float32 and taxonomy.is_cuda and taxonomy.numel() == 4 and taxonomy.is_contiguous()
    with torch.cuda.device(x.device):
        rc = lib.haff_gate_threshold_masks(x.data_ptr(), buf.data_ptr(), total, stride, ctypes.cast(ths, ctypes.c_void_p), n_th,
                                           int(on_value), _p(taxonomy), int(blank_class), _stream())
    check(rc, "haff_gate_threshold_masks")
    return buf[:, :total].reshape((n_th,) + tuple(x.shape))


def robot_heatmap(logits, jet):
    """fp32 [n, H, W] mask logits -> uint8 [n, H, W, 3] RGB: robot_demo.py's create_heatmap per plane (min-max to 0..255, truncate,
    JET through the device table jet uint8 [256, 3], the bit-exact 5x5 sigma-1 Gaussian blur)."""
    lib = load_library()
    _req(logits, "logits")
    assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 3
    assert jet.dtype == torch.uint8 and jet.is_cuda and jet.shape == (256, 3) and jet.is_contiguous()
    n, H, W = logits.shape
    ws = torch.empty((n * 512,), dtype=torch.float32, device=logits.device)
    out = torch.empty((n, H, W, 3), dtype=torch.uint8, device=logits.device)
    with torch.cuda.device(logits.device):
        rc = lib.haff_robot_heatmap(logits.data_ptr(), n, H, W, jet.data_ptr(), ws.data_ptr(), ws.numel(), out.data_ptr(), _stream())
    check(rc, "haff_robot_heatmap")
    return out


def robot_mask(logits, th, margins, mask=None, on_value=255, out=None):
    """fp32 [H0, W0] -> uint8 [H0 + top + bottom, W0 + left + right]: (logits > th) pasted at (left, top), ANDed with the lowest bit
    of mask (uint8 of the padded size, or None), times on_value. margins = (left, top, right, bottom); a mask of another size is
    refused by the library, as cv2.bitwise_and raises. out: a contiguous uint8 plane of the padded size to write into."""
    lib = load_library()
    _req(logits, "logits")
    assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 2
    left, top, right, bottom = (int(v) for v in margins)
    H0, W0 = logits.shape
    mh = mw = 0
    if mask is not None:
        _req(mask, "mask")
        assert mask.dtype == torch.uint8 and mask.is_contiguous() and mask.dim() == 2
        mh, mw = mask.shape
    out = _out(out, (max(H0 + top + bottom, 0), max(W0 + left + right, 0)), torch.uint8, logits.device)
    with torch.cuda.device(logits.device):
        rc = lib.haff_robot_mask(logits.data_ptr(), H0, W0, left, top, right, bottom, float(th), _p(mask), mh, mw, int(on_value),
                                 out.data_ptr(), _stream())
    check(rc, "haff_robot_mask")
    return out


def mask_quantile7(logits, need):
    """fp32 [n, H, W] mask logits -> fp32 [n, H, W]: per pixel the weighted upper quantile of its 7x7 neighbourhood (reflect-101,
    weights of OpenCV's 7-tap Gaussian table, total 65536): the largest tap with weight{taps >= it} >= need. `out > lt` is then
    gaussian.py's smoothing of the plane `logits > lt`, for every lt (postprocess.smooth_need gives need for its --threshold)."""
    lib = load_library()
    _req(logits, "logits")
    assert logits.dtype == torch.float32 and logits.is_contiguous() and logits.dim() == 3
    n, H, W = logits.shape
    out = torch.empty_like(logits)
    with torch.cuda.device(logits.device):
        rc = lib.haff_mask_quantile7(logits.data_ptr(), n, H, W, int(need), out.data_ptr(), _stream())
    check(rc, "haff_mask_quantile7")
    return out


def resample_u8(frames, out_hw, axis, bounds, coeffs):
    """One axis of Pillow's antialiased resampling on uint8 NHWC frames [B,H,W,3]; bounds/coeffs = device int32 tables."""
    lib = load_library()
    _req(frames, "frames")
    assert frames.dtype == torch.uint8 and frames.is_contiguous() and frames.dim() == 4 and frames.shape[3] == 3
    assert bounds.dtype == torch.int32 and coeffs.dtype == torch.int32 and bounds.is_cuda and coeffs.is_cuda
    B, H, W, _ = frames.shape
    oh, ow = out_hw
    n_out = ow if axis == 0 else oh
    assert bounds.shape == (n_out, 2) and coeffs.shape[0] == n_out and bounds.is_contiguous() and coeffs.is_contiguous()
    out = torch.empty((B, oh, ow, 3), dtype=torch.uint8, device=frames.device)
    with torch.cuda.device(frames.device):
        rc = lib.haff_resample_u8(frames.data_ptr(), out.data_ptr(), B, H, W, oh, ow, axis, bounds.data_ptr(), coeffs.data_ptr(),
                                  coeffs.shape[1], _stream())
    check(rc, "haff_resample_u8")
    return out


def clip_normalize_u8(frames, top, left, size, lut, out_dtype):
    """uint8 NHWC [B,H,W,3] window (top, left, size, size) -> [B,3,size,size] through the f32 [3,256] device LUT."""
    lib = load_library()
    _req(frames, "frames")
    assert frames.dtype == torch.uint8 and frames.is_contiguous() and frames.shape[3] == 3
    assert lut.dtype == torch.float32 and lut.is_cuda and lut.shape == (3, 256) and lut.is_contiguous()
    B, H, W, _ = frames.shape
    out = torch.empty((B, 3, size, size), dtype=out_dtype, device=frames.device)
    with torch.cuda.device(frames.device):
        rc = lib.haff_clip_normalize_u8(frames.data_ptr(), out.data_ptr(), B, H, W, int(top), int(left), int(size), lut.data_ptr(),
                                        _dt(out), _stream())
    check(rc, "haff_clip_normalize_u8")
    return out


FILL_MAX_VERTS, FILL_MAX_COORD = 4096, 32768   # haff_fill_contours_u8's host-checked limits (csrc/contour_fill.hip)


def contour_points(contour):
    """One OpenCV-style contour ([n,2] or [n,1,2], any number type) as cvlite.draw_contours_filled reads it: int32 [n,2]."""
    return np.ascontiguousarray(np.asarray(contour, dtype=np.int32).reshape(-1, 2))


def fill_contours_supported(contour):
    """Whether haff_fill_contours_u8 takes this polygon (vertex count and coordinate range); beyond that the caller fills on the host."""
    pts = contour_points(contour)
    return len(pts) <= FILL_MAX_VERTS and (len(pts) == 0 or int(abs(pts).max()) < FILL_MAX_COORD)


def fill_contours(planes, hw, device, out=None):
    """cvlite.draw_contours_filled for a batch of planes in one launch. planes: one list of contours per output plane;
    returns uint8 [len(planes), H, W] of 0 / 1 (zeroed by the call itself: `out` may hold anything)."""
    lib = load_library()
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("fill_contours runs in HBM (cuda device); the hot path has no CPU fallback")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    H, W = int(hw[0]), int(hw[1])
    polys, plane_of = [], []
    for i, contours in enumerate(planes):
        for c in contours or []:
            polys.append(contour_points(c))
            plane_of.append(i)
    n_poly, n_planes = len(polys), len(planes)
    off = np.zeros((n_poly + 1,), dtype=np.int32)
    if n_poly:
        off[1:] = np.cumsum([len(p) for p in polys])
    n_pts = int(off[-1])
    desc = torch.empty((2 * n_poly + 1 + 2 * n_pts,), dtype=torch.int32, pin_memory=True)
    d = desc.numpy()
    d[:n_poly + 1] = off
    d[n_poly + 1:2 * n_poly + 1] = plane_of
    if n_pts:
        d[2 * n_poly + 1:] = np.concatenate(polys, 0).reshape(-1)
    out = _out(out, (n_planes, H, W), torch.uint8, device)
    host = desc.data_ptr()
    with torch.cuda.device(device):
        dev = desc.to(device, non_blocking=True)
        rc = lib.haff_fill_contours_u8(host + 4 * (2 * n_poly + 1), host, host + 4 * (n_poly + 1), dev.data_ptr(), n_poly, n_planes,
                                       out.data_ptr(), H, W, _stream())
    check(rc, "haff_fill_contours_u8")
    return out


AUG_FLIP, AUG_JITTER = 1, 2            # the flag bits of csrc/frame_augment.hip
AUG_MAX_PIXELS = 1 << 24               # H * W per frame haff_jitter_stats_u8 / haff_augment_u8 take; beyond: the caller's host route


def augment_frames_supported(hw):
    """Whether the frame kernels take a frame of this (H, W); beyond that the caller augments it on the host."""
    return int(hw[0]) * int(hw[1]) <= AUG_MAX_PIXELS


def _aug_args(frames, flags, factors):
    _req(frames, "frames")
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[3] == 3 and frames.is_contiguous(), tuple(frames.shape)
    B = frames.shape[0]
    assert flags.dtype == torch.int32 and flags.is_contiguous() and tuple(flags.shape) == (B,) and flags.device == frames.device
    assert factors.dtype == torch.float32 and factors.is_contiguous() and tuple(factors.shape) == (B, 3)
    assert factors.device == frames.device
    return B, frames.shape[1], frames.shape[2]


def jitter_stats(frames, flags, factors, out=None):
    """haff_jitter_stats_u8: int64 [B] on the device = the sum of L over the brightness-scaled frame for every frame whose flags
    carry AUG_JITTER, 0 for the others (zeroed by the call itself: `out` may hold anything)."""
    lib = load_library()
    B, H, W = _aug_args(frames, flags, factors)
    out = _out(out, (B,), torch.int64, frames.device)
    with torch.cuda.device(frames.device):
        rc = lib.haff_jitter_stats_u8(frames.data_ptr(), B, H, W, flags.data_ptr(), factors.data_ptr(), out.data_ptr(), _stream())
    check(rc, "haff_jitter_stats_u8")
    return out


def augment_u8(frames, flags, factors, sums, out=None):
    """haff_augment_u8: the jittered and / or mirrored copy of uint8 [B,H,W,3] frames (`sums` from jitter_stats on the same arguments)."""
    lib = load_library()
    B, H, W = _aug_args(frames, flags, factors)
    assert sums.dtype == torch.int64 and sums.is_contiguous() and tuple(sums.shape) == (B,) and sums.device == frames.device
    out = _out(out, frames.shape, torch.uint8, frames.device)
    with torch.cuda.device(frames.device):
        rc = lib.haff_augment_u8(frames.data_ptr(), out.data_ptr(), B, H, W, flags.data_ptr(), factors.data_ptr(), sums.data_ptr(),
                                 _stream())
    check(rc, "haff_augment_u8")
    return out


def flip_planes(planes, flags, out=None):
    """haff_flip_planes_u8: uint8 [P,H,W] with the planes whose flags carry AUG_FLIP mirrored left-right and the others copied."""
    lib = load_library()
    _req(planes, "planes")
    assert planes.dtype == torch.uint8 and planes.dim() == 3 and planes.is_contiguous(), tuple(planes.shape)
    P, H, W = planes.shape
    assert flags.dtype == torch.int32 and flags.is_contiguous() and tuple(flags.shape) == (P,) and flags.device == planes.device
    out = _out(out, planes.shape, torch.uint8, planes.device)
    with torch.cuda.device(planes.device):
        rc = lib.haff_flip_planes_u8(planes.data_ptr(), out.data_ptr(), P, H, W, flags.data_ptr(), _stream())
    check(rc, "haff_flip_planes_u8")
    return out


def augment_table(augs, device):
    """The device arrays of the augment kernels from one `aug` dict per frame ({"flip": bool, "jitter": None | (fb, fc, fs)}, or None):
    int32 [B] flags and float32 [B,3] factors, uploaded together from one pinned buffer."""
    B = len(augs)
    host = torch.zeros((4 * B,), dtype=torch.float32, pin_memory=True)      # [flags B | factors 3 B]
    h = host.numpy()
    bits = h.view(np.int32)
    for i, a in enumerate(augs):
        if a:
            bits[i] = (AUG_FLIP if a["flip"] else 0) | (AUG_JITTER if a["jitter"] is not None else 0)
            if a["jitter"] is not None:
                h[B + 3 * i:B + 3 * i + 3] = a["jitter"]
    dev = host.to(device, non_blocking=True)
    return dev[:B].view(torch.int32), dev[B:].view(B, 3)


def augment_frames(frames, augs):
    """One `aug` dict per frame applied to uint8 [B,H,W,3] frames in HBM: the stats pass only when a frame is jittered, then the
    one augment pass. Returns a new tensor (the input is left as it is)."""
    flags, factors = augment_table(augs, frames.device)
    if any(a and a["jitter"] is not None for a in augs):
        sums = jitter_stats(frames, flags, factors)
    else:
        sums = torch.zeros((frames.shape[0],), dtype=torch.int64, device=frames.device)
    return augment_u8(frames, flags, factors, sums)


AUG_CROP = 4                           # the crop bit of csrc/frame_crop.hip (beside AUG_FLIP, which it shares)
CROP_MAX_SCALE = 4                     # per-axis down-scale S / out haff_crop_resample_u8 takes: at most 17 bicubic taps
_CROP_GEOM = 12                        # descriptor words per sample (include/haff_hip.h)
_crop_tables = {}                      # (S, out) -> int32 [out, 2 + ksize] rows (first, count, coefficients); filled by the prefetch thread


def crop_supported(hw, S):
    """Whether haff_crop_resample_u8 takes a sample of this (H, W) whose crop square has side S; beyond that the caller crops on
    the host."""
    H, W = int(hw[0]), int(hw[1])
    return H * W <= AUG_MAX_PIXELS and S <= CROP_MAX_SCALE * H and S <= CROP_MAX_SCALE * W


def crop_table(S, out):
    """One axis of Image.resize(BICUBIC) from S to `out` pixels as the crop kernel reads it: int32 [out, 2 + ksize] rows of
    (first input index, tap count, Pillow's 22-bit coefficients). Built on the host (Pillow normalises in double) and cached per
    (S, out); DeviceIngest's prefetch thread calls this ahead of the step."""
    from .preprocess import pil_bicubic_tables_fast
    key = (int(S), int(out))
    tab = _crop_tables.get(key)
    if tab is None:
        bounds, coeffs = pil_bicubic_tables_fast(*key)
        tab = np.ascontiguousarray(np.concatenate([bounds, coeffs], 1), dtype=np.int32)
        if len(_crop_tables) >= 512:       # every S a run meets, times two axes: bounded, oldest first
            _crop_tables.pop(next(iter(_crop_tables)))
        _crop_tables[key] = tab
    return tab


def crop_descriptor(boxes, flips, hw):
    """The pinned int32 descriptor of haff_crop_resample_u8 for samples of one (H, W): boxes[b] is aff_dataset.crop_box's dict or None
    (the sample is copied), flips[b] its mirror. Samples with one S share their tables."""
    H, W = int(hw[0]), int(hw[1])
    B = len(boxes)
    tabs, where, words = [], {}, B * _CROP_GEOM
    for box in boxes:
        if box is not None:
            for n_out in (W, H):
                key = (box["S"], n_out)
                if key not in where:
                    tab = crop_table(*key)
                    where[key] = (words, tab.shape[1] - 2)
                    tabs.append((words, tab))
                    words += tab.size
    desc = torch.zeros((words,), dtype=torch.int32, pin_memory=torch.cuda.is_available())
    d = desc.numpy()
    for b, (box, flip) in enumerate(zip(boxes, flips)):
        g = d[b * _CROP_GEOM:(b + 1) * _CROP_GEOM]
        g[7] = AUG_FLIP if flip else 0
        if box is not None:
            g[:7] = [box[k] for k in ("x0", "y0", "cw", "ch", "px", "py", "S")]
            g[7] |= AUG_CROP
            g[8:10], g[10:12] = where[(box["S"], W)], where[(box["S"], H)]
    for off, tab in tabs:
        d[off:off + tab.size] = tab.reshape(-1)
    return desc


def crop_resample(x, boxes, flips, out=None, desc=None):
    """haff_crop_resample_u8: uint8 [B,H,W,C] in HBM (C = 3 frames; C = 1 mask planes, non-zero in, 0 / 1 out) with sample b mirrored
    where flips[b] and then replaced by the object-centred view of boxes[b] (aff_dataset.crop_box of the MIRRORED sample; None: no
    crop), as aff_dataset.crop_image does it with Pillow. One launch; a new tensor. desc: crop_descriptor(boxes, flips, (H, W)) when
    the caller built it ahead. A geometry beyond crop_supported is refused (-2) before anything is enqueued."""
    lib = load_library()
    _req(x, "x")
    assert x.dtype == torch.uint8 and x.dim() == 4 and x.shape[3] in (1, 3) and x.is_contiguous(), tuple(x.shape)
    B, H, W, C = x.shape
    assert len(boxes) == B and len(flips) == B
    if desc is None:
        desc = crop_descriptor(boxes, flips, (H, W))
    assert desc.dtype == torch.int32 and desc.is_contiguous() and desc.device.type == "cpu" and desc.numel() >= B * _CROP_GEOM
    out = _out(out, x.shape, torch.uint8, x.device)
    with torch.cuda.device(x.device):
        dev = desc.to(x.device, non_blocking=True)
        rc = lib.haff_crop_resample_u8(x.data_ptr(), out.data_ptr(), B, H, W, C, desc.data_ptr(), dev.data_ptr(), desc.numel(), _stream())
    check(rc, "haff_crop_resample_u8")
    return out


SCORE_FRAME_WORDS = 16                  # haff_score_frame (include/haff_hip.h): 128 bytes as 16 int64 words
MAX_SIDE = 4096                         # kMaxSide of csrc/mask_score.hip, contour_hausdorff.hip and affordance_extract.hip
SCORE_MAX_SIDE, SCORE_MAX_THRESHOLDS = MAX_SIDE, 8


def score_masks(frames, logit_ths, device, out_counts=None, vis=None):
    """haff_score_masks on a packed descriptor table. frames: int64 [n, SCORE_FRAME_WORDS] (numpy or a CPU tensor, as
    scoring.pack_frames builds it; every pointer in it a device pointer the caller keeps alive until the call returns).
    Returns int32 [n, n_th, 4] on the device = {intersection, union, predicted area, ground-truth area} per frame and LOGIT
    threshold (zeroed by the call itself; the values are below 2^25). out_counts: a contiguous int32 [n, n_th, 4] to write into.
    vis: int64 [m, SCORE_FRAME_WORDS], the haff_score_vis records of scoring.pack_vis, appended to the same upload: a frame whose
    descriptor names record k (pack_frames' "vis" key) has its overlays drawn by a further launch behind the scoring one. None:
    the bytes uploaded and the launches of a call without overlays."""
    lib = load_library()
    device = torch.device(device)
    if device.type != "cuda":
        raise RuntimeError("score_masks runs in HBM (cuda device); the hot path has no CPU fallback")
    frames = torch.as_tensor(frames)
    assert frames.dtype == torch.int64 and frames.dim() == 2 and frames.shape[1] == SCORE_FRAME_WORDS and frames.shape[0] >= 1
    n, n_th = frames.shape[0], len(logit_ths)
    m = 0
    if vis is not None:
        vis = torch.as_tensor(vis)
        assert vis.dtype == torch.int64 and vis.dim() == 2 and vis.shape[1] == SCORE_FRAME_WORDS and vis.shape[0] >= 1
        m = vis.shape[0]
    host = torch.empty((n + m, SCORE_FRAME_WORDS), dtype=torch.int64, pin_memory=True)
    host[:n].copy_(frames)
    if m:
        host[n:].copy_(vis)
    named = int(host[:n].numpy().view(np.int32)[:, 29].max())   # the library reads record `named - 1` behind the frames: it must be there
    assert named <= m, f"a frame names overlay record {named} of {m}"
    if out_counts is None:
        out_counts = torch.empty((n, n_th, 4), dtype=torch.int32, device=device)
    assert out_counts.dtype == torch.int32 and out_counts.is_contiguous() and tuple(out_counts.shape) == (n, n_th, 4)
    assert out_counts.device.type == "cuda"
    ths = (ctypes.c_float * max(n_th, 1))(*[float(v) for v in logit_ths])
    with torch.cuda.device(out_counts.device):
        dev = host.to(out_counts.device, non_blocking=True)
        rc = lib.haff_score_masks(host.data_ptr(), dev.data_ptr(), n, ctypes.cast(ths, ctypes.c_void_p), n_th,
                                  out_counts.data_ptr(), _stream())
    check(rc, "haff_score_masks")
    return out_counts


HAUSDORFF_MAX_SIDE, HAUSDORFF_MAX_PLANES, HAUSDORFF_MAX_VERTICES = MAX_SIDE, 4096, 1 << 22   # csrc/contour_hausdorff.hip
HAUSDORFF_OVERFLOW, HAUSDORFF_FAULT = 0b0101, 0b1010     # result[:, 4]: either plane of the pair ran past max_vertices / hit a bound


def _u8_planes(planes):
    """The planes of a contour call as a list, checked (uint8 [H, W], contiguous, in HBM, on one device), and that device."""
    planes = list(planes)
    assert planes, "no planes"
    for p in planes:
        _req(p, "planes")
        assert p.dtype == torch.uint8 and p.dim() == 2 and p.is_contiguous(), (p.dtype, tuple(p.shape), p.is_contiguous())
        assert p.device == planes[0].device
    return planes, planes[0].device


def _plane_table(planes, extra_words=0):
    """The pinned int64 table of 16-byte haff_contour_plane descriptors {pointer, H, W} (include/haff_hip.h), with `extra_words`
    zeroed int64 words behind them."""
    host = torch.zeros((2 * len(planes) + extra_words,), dtype=torch.int64, pin_memory=True)
    h64 = host.numpy()
    h32 = h64.view(np.int32)
    for i, p in enumerate(planes):
        h64[2 * i] = p.data_ptr()
        h32[4 * i + 2], h32[4 * i + 3] = p.shape
    return host


def contour_hausdorff(planes, pairs, max_vertices=65536, return_vertices=False):
    """haff_contour_hausdorff: planes = uint8 CUDA tensors [H, W] (a list, or one [n, H, W] tensor), on where != 0; pairs = (bench,
    pred) indices into planes, two planes of one shape each. Returns int32 [n_pairs, 6] on the device = {bench vertices, pred
    vertices, d2(pred -> bench), d2(bench -> pred), flags, 0}: the squared directed Hausdorff distances between the vertex lists of
    `cvlite.find_contours_external(plane)[0]`, exact integers, both 0 when a side is empty or a flag is set. Only enqueues: no
    synchronisation, the caller keeps the planes alive until the stream has run. return_vertices: also int16 [n, max_vertices, 2]
    (x, y) in walk order (rows past a plane's count hold whatever the buffer held) and the int32 [n] vertex counts; True, or the
    uint8 CUDA buffer of at least 4 n max_vertices + 4 n bytes they are to be views of."""
    lib = load_library()
    planes, device = _u8_planes(planes)
    n, max_vertices = len(planes), int(max_vertices)
    pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int32).reshape(-1, 2))
    n_pairs = len(pairs)
    host = _plane_table(planes, extra_words=n_pairs)         # the int32 pairs lie behind the plane descriptors
    host.numpy().view(np.int32)[4 * n:4 * n + 2 * n_pairs] = pairs.reshape(-1)
    need = ctypes.c_long(0)
    check(lib.haff_contour_hausdorff_workspace(host.data_ptr(), n, max_vertices, ctypes.addressof(need)),
          "haff_contour_hausdorff_workspace")
    result = torch.empty((n_pairs, 6), dtype=torch.int32, device=device)
    verts = None
    if torch.is_tensor(return_vertices):
        verts, return_vertices = return_vertices, True
        assert verts.dtype == torch.uint8 and verts.is_contiguous() and verts.device == device
        assert verts.numel() >= n * max_vertices * 4 + n * 4
    elif return_vertices:
        verts = torch.empty((n * max_vertices * 4 + n * 4,), dtype=torch.uint8, device=device)
    with torch.cuda.device(device):
        ws = _workspace(device, need.value)
        dev = host.to(device, non_blocking=True)
        rc = lib.haff_contour_hausdorff(host.data_ptr(), dev.data_ptr(), n, host.data_ptr() + 16 * n, dev.data_ptr() + 16 * n, n_pairs,
                                        max_vertices, ws.data_ptr(), ws.numel(), _p(verts), result.data_ptr(), _stream())
    check(rc, "haff_contour_hausdorff")
    if not return_vertices:
        return result
    return (result, verts[:n * max_vertices * 4].view(torch.int16).reshape(n, max_vertices, 2),
            verts[n * max_vertices * 4:n * max_vertices * 4 + 4 * n].view(torch.int32))


EXTRACT_MAX_CONTOURS = 1 << 22                            # csrc/contour_hausdorff.hip kMaxContours
EXTRACT_OVERFLOW, EXTRACT_FAULT, EXTRACT_TOO_MANY = 1, 2, 4   # summary[:, 2]


def contour_extract(planes, max_contours=1024, max_vertices=65536, out=None):
    """haff_contour_extract: planes = uint8 CUDA tensors [H, W] (a list, or one [n, H, W] tensor), on where != 0, of any mix of
    shapes. Returns (summary, offsets, verts) on the device: int32 [n, 4] = {n_contours, n_vertices, flags, 0}, int32
    [n, max_contours + 1] (entry k = the first vertex of contour k, entry n_contours = the total) and int16 [n, max_vertices, 2]
    (x, y): every contour of `cvlite.find_contours_external(plane)`, in its order, back to back. A plane with a flag set
    (EXTRACT_OVERFLOW / EXTRACT_FAULT / EXTRACT_TOO_MANY) holds nothing of use in offsets and verts; what lies past a plane's
    n_contours + 1 offsets and n_vertices vertices is left as it was. Only enqueues: no synchronisation, the caller keeps the planes
    alive until the stream has run. out: the (summary, offsets, verts) tensors to write into."""
    lib = load_library()
    planes, device = _u8_planes(planes)
    n, max_contours, max_vertices = len(planes), int(max_contours), int(max_vertices)
    host = _plane_table(planes)
    need = ctypes.c_long(0)
    check(lib.haff_contour_extract_workspace(host.data_ptr(), n, max_contours, max_vertices, ctypes.addressof(need)),
          "haff_contour_extract_workspace")
    summary, offsets, verts = out if out is not None else (None, None, None)
    summary = _out(summary, (n, 4), torch.int32, device)
    offsets = _out(offsets, (n, max_contours + 1), torch.int32, device)
    verts = _out(verts, (n, max_vertices, 2), torch.int16, device)
    with torch.cuda.device(device):
        ws = _workspace(device, need.value)
        dev = host.to(device, non_blocking=True)
        rc = lib.haff_contour_extract(host.data_ptr(), dev.data_ptr(), n, max_contours, max_vertices, ws.data_ptr(), ws.numel(),
                                      verts.data_ptr(), offsets.data_ptr(), summary.data_ptr(), _stream())
    check(rc, "haff_contour_extract")
    return summary, offsets, verts


AFF_EXTRACT_ITEM_WORDS = 8              # haff_extract_item (include/haff_hip.h): 64 bytes as 8 int64 words
AFF_EXTRACT_MAX_SIDE, AFF_EXTRACT_MAX_K = MAX_SIDE, 31
AFF_EXTRACT_HAND, AFF_EXTRACT_GREY = 1, 2   # stats[:, 7]: a hand was ANDed in / `a` holds a value other than 0 and 255
AFF_EXTRACT_STATS = ("nonzero_a", "nonzero_out", "sum_a", "min_row", "max_row", "min_col", "max_col", "flags")


def nearest_pad_tables(hand_hw, out_hw, device=None):
    """The gather tables of `cv2.resize(pad_image(hand), (W, H), interpolation=INTER_NEAREST)` for a hand mask of shape hand_hw and a
    plane of shape out_hw = (H, W): int32 (col [W], row [H]), the hand's own column / row each output column / row reads, -1 for
    the padding. pad_image (affordance_extraction_preparation.py:53-61) pads to the square of side S = max(Hh, Wh): a portrait
    mask (Hh > Wh) on the LEFT, any other on the TOP. resizeNN computes its indices in double, and not as the exact rational floor:
    p = min(floor(x * (1.0 / (D / S))), S - 1) with the division and the reciprocal in IEEE double in that order (D = 34, S = 6,
    x = 17 reads 2, not 17 * 6 // 34 = 3). The reference skips the resize when the padded hand already has the plane's shape: the
    formula gives the identity for D == S, which is asserted here. CPU tensors, or on `device`."""
    Hh, Wh = int(hand_hw[0]), int(hand_hw[1])
    H, W = int(out_hw[0]), int(out_hw[1])
    assert Hh >= 1 and Wh >= 1 and H >= 1 and W >= 1, (hand_hw, out_hw)
    S = max(Hh, Wh)

    def axis(D, pad):
        inv = 1.0 / (D / S)                                   # Python floats are IEEE doubles
        p = np.minimum(np.floor(np.arange(D, dtype=np.float64) * inv), S - 1).astype(np.int64)
        if D == S:
            assert np.array_equal(p, np.arange(S)), "the nearest table of an unchanged length is the identity"
        p = p - pad
        p[p < 0] = -1
        return torch.from_numpy(p.astype(np.int32))

    col, row = axis(W, S - Wh if Hh > Wh else 0), axis(H, 0 if Hh > Wh else S - Hh)
    if device is not None:
        col, row = col.to(device), row.to(device)
    return col, row


def affordance_extract(items, k, stats=None):
    """haff_affordance_extract on a batch of any mix of shapes. items: a list of (plane, hand, tables, out): plane = uint8 CUDA [H, W];
    hand = None or uint8 CUDA [Hh, Wh] with tables = (col int32 [W], row int32 [H]) on the device as nearest_pad_tables builds them
    (items of one geometry may share them); out = None (statistics only) or uint8 CUDA [H, W]. k: the dilation's side, 1..31.
    a = plane & hand[row][:, col] (bitwise; 0 in the padding), out = 255 where the k x k window (anchor k // 2) holds a non-zero a.
    Returns int64 [n, 8] on the device, columns AFF_EXTRACT_STATS, zeroed by the call itself. Only enqueues: no synchronisation, the
    caller keeps the tensors alive until the stream has run. Every refusal is raised before anything is written."""
    lib = load_library()
    items = list(items)
    if not items:
        raise ValueError("affordance_extract: no items")
    k = int(k)
    if not 1 <= k <= AFF_EXTRACT_MAX_K:
        raise ValueError(f"affordance_extract: k = {k} is outside 1..{AFF_EXTRACT_MAX_K}")

    def u8(t, name, i):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f"affordance_extract: item {i}: {name} must live in HBM (cuda tensor); there is no CPU fallback")
        if t.dtype != torch.uint8:
            raise TypeError(f"affordance_extract: item {i}: {name} is {t.dtype}, not uint8")
        if t.dim() != 2 or t.numel() == 0:
            raise ValueError(f"affordance_extract: item {i}: {name} has shape {tuple(t.shape)}, not [H, W]")
        if not t.is_contiguous():
            raise ValueError(f"affordance_extract: item {i}: {name} is not contiguous")
        if max(t.shape) > AFF_EXTRACT_MAX_SIDE:
            raise ValueError(f"affordance_extract: item {i}: {name} has a side over {AFF_EXTRACT_MAX_SIDE}")

    def table(t, name, i, length):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise RuntimeError(f"affordance_extract: item {i}: {name} table must live in HBM (cuda tensor)")
        if t.dtype != torch.int32:
            raise TypeError(f"affordance_extract: item {i}: {name} table is {t.dtype}, not int32")
        if not t.is_contiguous():
            raise ValueError(f"affordance_extract: item {i}: {name} table is not contiguous")
        if t.dim() != 1 or t.numel() != length:
            raise ValueError(f"affordance_extract: item {i}: {name} table has shape {tuple(t.shape)}, not [{length}]")

    n = len(items)
    host = torch.zeros((n, AFF_EXTRACT_ITEM_WORDS), dtype=torch.int64, pin_memory=True)
    h64 = host.numpy()
    h32 = h64.view(np.int32)
    device = None
    for i, (plane, hand, tables, out) in enumerate(items):
        u8(plane, "plane", i)
        device = plane.device if device is None else device
        H, W = plane.shape
        Hh = Wh = 0
        if hand is not None:
            u8(hand, "hand", i)
            if tables is None or len(tables) != 2:
                raise ValueError(f"affordance_extract: item {i}: a hand needs its (col, row) tables")
            table(tables[0], "col", i, W)
            table(tables[1], "row", i, H)
            Hh, Wh = hand.shape
        if out is not None:
            u8(out, "out", i)
            if tuple(out.shape) != (H, W):
                raise ValueError(f"affordance_extract: item {i}: out has shape {tuple(out.shape)}, the plane {(H, W)}")
        for t in (hand, out) + (tuple(tables) if hand is not None else ()):
            if t is not None and t.device != device:
                raise RuntimeError(f"affordance_extract: item {i}: tensors on {t.device} and {device}")
        if plane.device != device:
            raise RuntimeError(f"affordance_extract: item {i}: tensors on {plane.device} and {device}")
        h64[i, 0] = plane.data_ptr()
        h64[i, 1] = _p(hand)
        h64[i, 2] = tables[0].data_ptr() if hand is not None else 0
        h64[i, 3] = tables[1].data_ptr() if hand is not None else 0
        h64[i, 4] = _p(out)
        h32[i, 10:14] = (H, W, Hh, Wh)
    stats = _out(stats, (n, 8), torch.int64, device)
    with torch.cuda.device(device):
        dev = host.to(device, non_blocking=True)
        rc = lib.haff_affordance_extract(host.data_ptr(), dev.data_ptr(), n, k, stats.data_ptr(), _stream())
    check(rc, "haff_affordance_extract")
    return stats


PNG_MAX_SIDE, PNG_MAX_PLANES = MAX_SIDE, 4096            # csrc/png_encode.hip


def png_block_bound(H, W):
    """The most bytes the block of an H x W plane can take (include/haff_io.h): every byte a 9-bit literal."""
    return (10 + 9 * (W + 1) * H + 7) // 8


def png_measure(planes):
    """haff_png_measure: planes = uint8 CUDA tensors [H, W] of any mix of shapes (a list, or one [n, H, W] tensor), any values.
    Returns (table, job): table int32 [n, 4] on the device, to be read as uint32 = {byte offset of the plane's DEFLATE block in
    png_emit's output, its byte length, the Adler-32 of the plane's scanlines, 0}; job = what png_emit needs beside the table as the
    host read it (the descriptors, the workspace with every scanline's bit offset). Only enqueues."""
    lib = load_library()
    planes, device = _u8_planes(planes)
    n = len(planes)
    host = _plane_table(planes)                          # haff_png_plane = haff_contour_plane's layout: {pointer, H, W}
    need = ctypes.c_long(0)
    check(lib.haff_png_workspace(host.data_ptr(), n, ctypes.addressof(need)), "haff_png_workspace")
    table = torch.empty((n, 4), dtype=torch.int32, device=device)
    ws = torch.empty((max(need.value, 16),), dtype=torch.uint8, device=device)   # its own: it lives until png_emit has run
    with torch.cuda.device(device):
        dev = host.to(device, non_blocking=True)
        rc = lib.haff_png_measure(host.data_ptr(), dev.data_ptr(), n, ws.data_ptr(), ws.numel(), table.data_ptr(), _stream())
    check(rc, "haff_png_measure")
    return table, (planes, host, dev, ws, table)


def png_emit(job, table_host, out=None):
    """haff_png_emit: job = png_measure's, table_host = its table as a uint32 numpy array [n, 4] read back by the caller. Returns the
    uint8 CUDA tensor of exactly the size the table implies (the last plane's offset + length, rounded up to 4), or `out` (uint8,
    contiguous, at least that size; only that many bytes are written): every plane's block at its offset, zeros between a block's end
    and the next offset. Only enqueues."""
    lib = load_library()
    planes, host, dev, ws, table = job
    th = np.ascontiguousarray(table_host, dtype=np.uint32)
    assert th.shape == (len(planes), 4), th.shape
    total = int(th[-1, 0]) + (int(th[-1, 1]) + 3) // 4 * 4
    device = table.device
    if out is None:
        out = torch.empty((total,), dtype=torch.uint8, device=device)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.device == device
    with torch.cuda.device(device):
        rc = lib.haff_png_emit(host.data_ptr(), dev.data_ptr(), len(planes), ws.data_ptr(), ws.numel(), th.ctypes.data, table.data_ptr(),
                               out.data_ptr(), out.numel(), _stream())
    check(rc, "haff_png_emit")
    return out
