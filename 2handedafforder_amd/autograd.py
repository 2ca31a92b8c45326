"""Differentiable ops of the LoRA fine-tune path: torch.autograd.Function shells whose forward AND backward are
hand-written HIP kernels (csrc/train.hip + the GEMM / norm kernels). torch.autograd only records the graph and
routes gradients (plumbing); no torch arithmetic runs in these Functions.

Reference semantics: LISAForCausalLM.model_forward (2Haff/model/LISA.py:175-430), peft LoRA on q_proj/v_proj
(train_ds.py:217-231), transformers LlamaDecoderLayer / CrossEntropyLoss (llava_llama.py:93-118).
Contractions in backward reuse the NT GEMM (C = A.W^T): dX = dY.W via W^T, dW = dY^T.X via transposed operands.
"""
import torch
from torch.autograd import Function

from . import ops
from .lib import check, load_library


def _dt(t):
    return ops._dt(t)


def _s():
    return ops._stream()


def _call(name, *args):
    """The library's entry point `name` on the current stream (its last argument), checked under that name."""
    check(getattr(load_library(), name)(*args, _s()), name)


def _pad8(n):
    return (n + 7) // 8 * 8


HALF = (torch.bfloat16, torch.float16)   # the 16-bit training dtypes: bf16 (throughput mode) and fp16 (the --precision fp16 mode)


def _fn16(lib, name, dtype):
    """The entry point of a 16-bit training kernel for dtype: the bf16 one, or its *_f16 sibling (same arguments) for fp16."""
    if dtype == torch.float16:
        return getattr(lib, name.replace("_bf16", "_f16") if "_bf16" in name else name + "_f16")
    return getattr(lib, name)


def _call16(name, dtype, *args):
    """_call for a 16-bit training kernel: the entry point `name` for bf16, its *_f16 sibling for fp16 (_fn16)."""
    check(_fn16(load_library(), name, dtype)(*args, _s()), name)


def _f32_workspace(fn, dev, *shape):
    """The f32 partials of a product contracted over rows: as many values as the library's fn(*shape) asks for."""
    n_ws = getattr(load_library(), fn)(*shape)
    assert n_ws > 0
    return torch.empty((n_ws,), dtype=torch.float32, device=dev)


def scale_dev(a, alpha, per_row=False):
    """a * alpha with alpha a DEVICE fp32 scalar (or one value per row of the 2-D a): the multiply runs in fp32 inside the kernel —
    a torch multiply would first round the 0-dim upstream gradient to a's dtype (bf16)."""
    a = a.contiguous()
    if a.numel() == 0:   # empty in, empty out (the torch multiply this replaced accepted it; the kernel entry refuses cols = 0)
        return a.clone()
    alpha = alpha.detach().to(torch.float32).contiguous()
    rows, cols = (a.shape[0], a.numel() // a.shape[0]) if per_row else (1, a.numel())
    assert alpha.numel() == (rows if per_row else 1) and alpha.device == a.device
    out = torch.empty_like(a)
    _call("haff_scale_dev", a.data_ptr(), out.data_ptr(), rows, cols, alpha.data_ptr(), 1 if per_row else 0, _dt(a))
    return out


# ------------------------------------------------------------------------------------------------------------------
# raw (non-differentiable) wrappers of csrc/train.hip
# ------------------------------------------------------------------------------------------------------------------
def transpose(x, Rp=None, Cp=None):
    """x [..., R, C] (any batch strides, unit inner stride) -> [Z, Cp, Rp] contiguous, zero padded."""
    if x.dim() == 2:
        x = x.unsqueeze(0)
    lead = x.shape[:-2]
    R, C = x.shape[-2], x.shape[-1]
    assert x.stride(-1) == 1
    Rp = R if Rp is None else Rp
    Cp = C if Cp is None else Cp
    if len(lead) == 1:
        nbo, nbi, so, si = lead[0], 1, x.stride(0), 0
    elif len(lead) == 2:
        nbo, nbi, so, si = lead[0], lead[1], x.stride(0), x.stride(1)
    else:
        raise ValueError("transpose supports at most two batch dims")
    out = torch.empty((nbo * nbi, Cp, Rp), dtype=x.dtype, device=x.device)
    _call("haff_transpose", x.data_ptr(), x.stride(-2), so, si, out.data_ptr(), R, C, Rp, Cp, nbo, nbi, _dt(x))
    return out


def bgemm(a, w, out=None, out_dtype=None):
    """Batched NT product: a [Zo,Zi,M,K], w [Zo,Zi,N,K] (strided views, unit inner stride) -> out [Zo,Zi,M,N]
    (contiguous unless `out` is a strided view with unit inner stride)."""
    Zo, Zi, M, K = a.shape
    N = w.shape[2]
    assert w.shape[0] == Zo and w.shape[1] == Zi and w.shape[3] == K and a.stride(3) == 1 and w.stride(3) == 1
    if out_dtype is None:
        out_dtype = a.dtype
    if out is None:
        out = torch.empty((Zo, Zi, M, N), dtype=out_dtype, device=a.device)
    assert out.stride(3) == 1
    args = (a.data_ptr(), a.stride(2), a.stride(0), a.stride(1), w.data_ptr(), w.stride(2), w.stride(0), w.stride(1), out.data_ptr(),
            out.stride(2), out.stride(0), out.stride(1), Zo, Zi, M, N, K)
    if a.dtype in HALF:
        assert w.dtype == a.dtype
        _call16("haff_gemm_bf16_batched", a.dtype, *args, 1 if out.dtype == torch.float32 else 0)
    else:
        assert out.dtype == torch.float32
        _call("haff_gemm_f32_batched", *args)
    return out


def gemm_tn_supported(a, b):
    return (a.dtype in HALF and b.dtype == a.dtype and a.dim() == 2 and b.dim() == 2 and a.shape[0] == b.shape[0]
            and a.stride(1) == 1 and b.stride(1) == 1 and a.shape[1] % 8 == 0 and b.shape[1] % 8 == 0 and a.stride(0) % 8 == 0
            and b.stride(0) % 8 == 0 and a.data_ptr() % 16 == 0 and b.data_ptr() % 16 == 0)


def gemm_tn(a, b, out_dtype=None):
    """a [M, N1], b [M, N2] (bf16 or fp16, row strides free) -> a^T @ b [N1, N2]: the contraction runs over the ROWS, no transposed copy
    of either operand (haff_gemm_tn_bf16 / _f16)."""
    assert gemm_tn_supported(a, b)
    M, N1 = a.shape
    N2 = b.shape[1]
    out = torch.empty((N1, N2), dtype=out_dtype or a.dtype, device=a.device)
    ws = _f32_workspace("haff_gemm_tn_workspace_elems", a.device, M, N1, N2)
    _call16("haff_gemm_tn_bf16", a.dtype, a.data_ptr(), a.stride(0), b.data_ptr(), b.stride(0), M, N1, N2, ws.data_ptr(), ws.numel(), out.data_ptr(),
            1 if out.dtype == torch.float32 else 0)
    return out


ORDERED_REDUCTIONS = True   # False: the fp32-atomic forms of rounds 1-3 (A/B; run-to-run differences in the last bits and beyond)


def _reduce_partials(partials, out, n_out, n_parts, out_inner, part_stride, group_stride, accumulate):
    _call("haff_reduce_partials", partials.data_ptr(), out.data_ptr(), n_out, n_parts, out_inner, part_stride, group_stride, 1 if accumulate else 0)


def colsum(x2d):
    """Column sums (bias / norm-weight gradients), fp32 [C]. Ordered form: per-row-block partial sums, added in block order."""
    lib = load_library()
    x2d = x2d.contiguous()
    R, C = x2d.shape
    if R == 0 or C == 0:   # no rows: the sums are zero (the kernel entries refuse empty inputs)
        return torch.zeros((C,), dtype=torch.float32, device=x2d.device)
    if not ORDERED_REDUCTIONS:
        out = torch.zeros((C,), dtype=torch.float32, device=x2d.device)
        _call("haff_colsum", x2d.data_ptr(), out.data_ptr(), R, C, _dt(x2d))
        return out
    parts = lib.haff_colsum_parts(R)
    partials = torch.empty((parts, C), dtype=torch.float32, device=x2d.device)
    _call("haff_colsum_partials", x2d.data_ptr(), partials.data_ptr(), R, C, _dt(x2d))
    out = torch.empty((C,), dtype=torch.float32, device=x2d.device)
    _reduce_partials(partials, out, C, parts, C, C, 0, False)
    return out


def _mul(a, b):
    a, b = a.contiguous(), b.contiguous()
    out = torch.empty_like(a)
    _call("haff_mul", a.data_ptr(), b.data_ptr(), out.data_ptr(), a.numel(), _dt(a))
    return out


def axpby(a, b, alpha, beta):
    a = a.contiguous()
    out = torch.empty_like(a)
    bp = 0
    if b is not None:
        b = b.contiguous()
        bp = b.data_ptr()
    _call("haff_axpby", a.data_ptr(), bp, out.data_ptr(), a.numel(), float(alpha), float(beta), _dt(a))
    return out


# ------------------------------------------------------------------------------------------------------------------
# Functions
# ------------------------------------------------------------------------------------------------------------------
TN_WEIGHT_GRADIENTS = True   # False: dW through haff_transpose + the NT product (A/B, tests)


class FrozenWeight:
    """A frozen Linear weight as the nodes below take it in place of the tensors (w, w_t): w() is W [N, K] for the forward product,
    w_t() is W^T [K, N] (or [K, roundup(N, 8)] with zero pad columns) for dX = dY . W. Here both are resident tensors: the bf16 /
    fp32 / fp16 trainers, which get back the very tensors they passed in.

    The contract a node keeps, so that Nf4FrozenWeight can stand in: what w() / w_t() return is used AT ONCE, on the stream it was
    asked for on, and is never put in ctx.save_for_backward. The node keeps the FrozenWeight itself (ctx.frozen) and asks again in
    backward, immediately before the dX product."""

    def __init__(self, w, w_t=None):
        self._w, self._wt = w, w_t
        self.shape, self.dtype, self.device = tuple(w.shape), w.dtype, w.device

    def w(self):
        return self._w

    def w_t(self):
        if self._wt is None:
            self._wt = transpose(self._w, Rp=_pad8(self.shape[0]))[0]
        return self._wt


class Nf4FrozenWeight(FrozenWeight):
    """A frozen NF4 Linear (quant.Nf4Weight: packed codes + absmax, the only resident form). Every w() / w_t() dequantises into the
    scratch buffer of its shape — ONE [N, K] and ONE [K, roundup(N, 8)] f16 buffer per distinct projection shape, shared by all
    layers (scratch: {("w" | "w_t", (N, K)): tensor}). The tensor handed out holds another layer's weights after the next call on
    the same shape, and the kernels write it through ctypes, behind autograd's version counters: hence FrozenWeight's contract."""

    def __init__(self, q, scratch):
        self.q, self._scratch = q, scratch
        self.shape, self.dtype, self.device = tuple(q.shape), torch.float16, q.packed.device

    def w(self):
        return self.q.dequant(out=self._scratch["w", self.shape])

    def w_t(self):
        return self.q.dequant_t(out=self._scratch["w_t", self.shape])


def frozen(w, w_t=None):
    """The FrozenWeight of a node's (w, w_t) arguments: w itself when it is one already, else the two resident tensors."""
    return w if isinstance(w, FrozenWeight) else FrozenWeight(w, w_t)


class LinearFn(Function):
    """y = x @ w.T + bias (+ resid). w_t: optional precomputed w.T (frozen weights keep one resident). w may be a FrozenWeight
    (the trainer's frozen Llama projections): no dW, W^T from w.w_t() in backward."""

    @staticmethod
    def forward(ctx, x, w, bias, resid, w_t):
        x2 = x if x.stride(1) == 1 else x.contiguous()
        ctx.frozen = w if isinstance(w, FrozenWeight) else None
        ctx.has_bias = bias is not None
        ctx.has_resid = resid is not None
        if ctx.frozen is not None:
            y = ops.linear(x2, w.w(), bias=bias, resid=resid)
            none = torch.empty(0, device=x.device)
            ctx.save_for_backward(x2, none, none)
            return y
        y = ops.linear(x2, w, bias=bias, resid=resid)
        ctx.save_for_backward(x2, w, w_t if w_t is not None else torch.empty(0, device=x.device))
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, w_t = ctx.saved_tensors
        dy = dy.contiguous()
        dx = dw = db = dres = None
        M, K = x.shape
        N = w.shape[0] if ctx.frozen is None else ctx.frozen.shape[0]
        if ctx.needs_input_grad[0]:
            if ctx.frozen is not None:
                w_t = ctx.frozen.w_t()
            elif w_t.numel() == 0:
                w_t = transpose(w, Rp=_pad8(N))[0]  # [K, Np]
            dyk = dy
            if w_t.shape[1] != N:  # K-dim of this product is N: pad dy's columns with zeros
                dyk = torch.zeros((M, w_t.shape[1]), dtype=dy.dtype, device=dy.device)
                dyk[:, :N] = dy
            dx = ops.linear(dyk, w_t)
        if ctx.needs_input_grad[1]:
            if TN_WEIGHT_GRADIENTS and M >= 16 and gemm_tn_supported(dy, x):
                dw = gemm_tn(dy, x)              # [N, K] = dy^T . x, both operands read as they lie (csrc/gemm_tn.hip)
            else:
                Mp = _pad8(M)
                dy_t = transpose(dy, Rp=Mp)[0]   # [N, Mp]
                x_t = transpose(x, Rp=Mp)[0]     # [K, Mp]
                dw = ops.linear(dy_t, x_t)       # [N, K]
        if ctx.has_bias and ctx.needs_input_grad[2]:
            db = colsum(dy)
        if ctx.has_resid and ctx.needs_input_grad[3]:
            dres = dy
        return dx, dw, db, dres, None


def linear(x, w, bias=None, resid=None, w_t=None):
    return LinearFn.apply(x, w, bias, resid, w_t)


class ActFn(Function):
    @staticmethod
    def forward(ctx, x, act):
        x = x.contiguous()
        y = torch.empty_like(x)
        _call("haff_act_fwd", x.data_ptr(), y.data_ptr(), x.numel(), act, _dt(x))
        ctx.save_for_backward(x)
        ctx.act = act
        return y

    @staticmethod
    def backward(ctx, dy):
        (x,) = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        _call("haff_act_bwd", x.data_ptr(), dy.data_ptr(), dx.data_ptr(), x.numel(), ctx.act, _dt(x))
        return dx, None


def act(x, code):
    return ActFn.apply(x, code)


class SwigluFn(Function):
    """gu [M, 2F] in the interleaved [gate x16 | up x16] column layout -> silu(gate) * up [M, F]."""

    @staticmethod
    def forward(ctx, gu):
        gu = gu.contiguous()
        M, F2 = gu.shape
        y = torch.empty((M, F2 // 2), dtype=gu.dtype, device=gu.device)
        _call("haff_swiglu_fwd", gu.data_ptr(), y.data_ptr(), M, F2 // 2, _dt(gu))
        ctx.save_for_backward(gu)
        return y

    @staticmethod
    def backward(ctx, dy):
        (gu,) = ctx.saved_tensors
        dy = dy.contiguous()
        dgu = torch.empty_like(gu)
        _call("haff_swiglu_bwd", gu.data_ptr(), dy.data_ptr(), dgu.data_ptr(), gu.shape[0], gu.shape[1] // 2, _dt(gu))
        return dgu


swiglu = SwigluFn.apply


class AddFn(Function):
    @staticmethod
    def forward(ctx, a, b):
        return axpby(a, b, 1.0, 1.0)

    @staticmethod
    def backward(ctx, dy):
        return dy, dy


add = AddFn.apply


class ScaleFn(Function):
    @staticmethod
    def forward(ctx, a, alpha):
        ctx.alpha = alpha
        return axpby(a, None, alpha, 0.0)

    @staticmethod
    def backward(ctx, dy):
        return axpby(dy, None, ctx.alpha, 0.0), None


scale = ScaleFn.apply


class AddBcastFn(Function):
    """out[r] = a[r] + b[r % mod] with b constant (positional encodings)."""

    @staticmethod
    def forward(ctx, a, b, mod):
        return ops.add_bcast(a.contiguous(), b, mod=mod)

    @staticmethod
    def backward(ctx, dy):
        return dy, None, None


add_const = AddBcastFn.apply


class LayerNormFn(Function):
    @staticmethod
    def forward(ctx, x, w, b, eps):
        x = x.contiguous()
        ctx.save_for_backward(x, w)
        ctx.eps = eps
        return ops.layernorm(x, w, b, eps)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        need_w = ctx.needs_input_grad[1]
        dyx = torch.empty(x.shape, dtype=torch.float32, device=x.device) if need_w else None
        _call("haff_norm_bwd", x.data_ptr(), dy.data_ptr(), w.data_ptr(), dx.data_ptr(), 0 if dyx is None else dyx.data_ptr(),
              x.shape[0], x.shape[1], float(ctx.eps), 0, _dt(x))
        dw = colsum(dyx) if need_w else None
        db = colsum(dy) if ctx.needs_input_grad[2] else None
        return dx, dw, db, None


layernorm = LayerNormFn.apply


class RMSNormFn(Function):
    @staticmethod
    def forward(ctx, x, w, eps):
        x = x.contiguous()
        ctx.save_for_backward(x, w)
        ctx.eps = eps
        return ops.rmsnorm(x, w, eps)

    @staticmethod
    def backward(ctx, dy):
        x, w = ctx.saved_tensors
        dy = dy.contiguous()
        dx = torch.empty_like(x)
        _call("haff_norm_bwd", x.data_ptr(), dy.data_ptr(), w.data_ptr(), dx.data_ptr(), 0, x.shape[0], x.shape[1], float(ctx.eps), 1, _dt(x))
        return dx, None, None


rmsnorm = RMSNormFn.apply


class ResidRMSNormFn(Function):
    """x -> (x, rmsnorm(x)) for a pre-norm residual block (transformers' LlamaDecoderLayer: h = norm(x); x_new = x + f(h)): the
    stream is handed on beside its normalised copy, so that backward sees BOTH gradients of x — the one that arrives along the
    residual branch and the norm's — and adds them inside the norm adjoint kernel (haff_norm_bwd_add): one pass instead of the
    adjoint + autograd's separate accumulation add (340 such adds per fine-tune step in round 4's profile)."""

    @staticmethod
    def forward(ctx, x, w, eps):
        x = x.contiguous()
        ctx.save_for_backward(x, w)
        ctx.eps = eps
        return x.view_as(x), ops.rmsnorm(x, w, eps)

    @staticmethod
    def backward(ctx, g_x, g_h):
        x, w = ctx.saved_tensors
        if g_h is None:
            return g_x, None, None
        g_h = g_h.contiguous()
        dx = torch.empty_like(x)
        if g_x is None:
            _call("haff_norm_bwd", x.data_ptr(), g_h.data_ptr(), w.data_ptr(), dx.data_ptr(), 0, x.shape[0], x.shape[1], float(ctx.eps), 1, _dt(x))
        else:
            g_x = g_x.contiguous()
            _call("haff_norm_bwd_add", x.data_ptr(), g_h.data_ptr(), w.data_ptr(), g_x.data_ptr(), dx.data_ptr(), 0, x.shape[0], x.shape[1],
                  float(ctx.eps), 1, _dt(x))
        return dx, None, None


resid_rmsnorm = ResidRMSNormFn.apply
FUSED_RESID_NORM = True   # False: rmsnorm + autograd's own gradient add (A/B, tests)


class RopeFn(Function):
    """x [rows, H*d] (rows = B*T, position = row % T) -> rotated copy."""

    @staticmethod
    def forward(ctx, x, cos_sin, T, H, d):
        x = x.contiguous()
        y = torch.empty_like(x)
        _call("haff_rope", x.data_ptr(), x.stride(0), y.data_ptr(), y.stride(0), cos_sin.data_ptr(), x.shape[0], T, H, d, 0, 0, _dt(x))
        ctx.save_for_backward(cos_sin)
        ctx.dims = (T, H, d)
        return y

    @staticmethod
    def backward(ctx, dy):
        (cos_sin,) = ctx.saved_tensors
        T, H, d = ctx.dims
        dy = dy.contiguous()
        dx = torch.empty_like(dy)
        _call("haff_rope", dy.data_ptr(), dy.stride(0), dx.data_ptr(), dx.stride(0), cos_sin.data_ptr(), dy.shape[0], T, H, d, 0, 1, _dt(dy))
        return dx, None, None, None, None


rope = RopeFn.apply


class AttentionFn(Function):
    """softmax(scale * q k^T [+ causal]) v with materialised probabilities (training sequences are a few hundred
    tokens: P for one layer is tens of MB in 288 GB of HBM). q [B,Nq,H*d], k/v [B,Nk,H*d] token-major -> [B,Nq,H*d]."""

    @staticmethod
    def forward(ctx, q, k, v, H, scale_, causal):
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        B, Nq, HD = q.shape
        Nk = k.shape[1]
        d = HD // H
        q4 = q.view(B, Nq, H, d).permute(0, 2, 1, 3)
        k4 = k.view(B, Nk, H, d).permute(0, 2, 1, 3)
        v4 = v.view(B, Nk, H, d).permute(0, 2, 1, 3)
        Nkp = _pad8(Nk)
        s = bgemm(q4, k4, out_dtype=torch.float32)                       # [B,H,Nq,Nk]
        p = torch.empty((B, H, Nq, Nkp), dtype=q.dtype, device=q.device)
        _call("haff_softmax_fwd", s.data_ptr(), Nk, p.data_ptr(), Nkp, B * H * Nq, Nq, Nk, float(scale_), 1 if causal else 0, Nk - Nq, _dt(q))
        vt = transpose(v4, Rp=Nkp).view(B, H, d, Nkp)                    # [B,H,d,Nkp]
        out = torch.empty((B, Nq, HD), dtype=q.dtype, device=q.device)
        bgemm(p, vt, out=out.view(B, Nq, H, d).permute(0, 2, 1, 3))
        ctx.save_for_backward(q, k, v, p)
        ctx.cfg = (H, float(scale_), Nk)
        return out

    @staticmethod
    def backward(ctx, do):
        q, k, v, p = ctx.saved_tensors
        H, scale_, Nk = ctx.cfg
        do = do.contiguous()
        B, Nq, HD = q.shape
        d = HD // H
        Nkp, Nqp = p.shape[3], _pad8(Nq)
        q4 = q.view(B, Nq, H, d).permute(0, 2, 1, 3)
        k4 = k.view(B, Nk, H, d).permute(0, 2, 1, 3)
        v4 = v.view(B, Nk, H, d).permute(0, 2, 1, 3)
        do4 = do.view(B, Nq, H, d).permute(0, 2, 1, 3)
        dp = bgemm(do4, v4, out_dtype=torch.float32)                     # [B,H,Nq,Nk]
        ds = torch.empty_like(p)
        _call("haff_softmax_bwd", p.data_ptr(), Nkp, dp.data_ptr(), Nk, ds.data_ptr(), B * H * Nq, Nk, scale_, _dt(p))
        kt = transpose(k4, Rp=Nkp).view(B, H, d, Nkp)
        dq = torch.empty_like(q)
        bgemm(ds, kt, out=dq.view(B, Nq, H, d).permute(0, 2, 1, 3))
        ds_t = transpose(ds[..., :Nk], Rp=Nqp).view(B, H, Nk, Nqp)
        p_t = transpose(p[..., :Nk], Rp=Nqp).view(B, H, Nk, Nqp)
        qt = transpose(q4, Rp=Nqp).view(B, H, d, Nqp)
        dot = transpose(do4, Rp=Nqp).view(B, H, d, Nqp)
        dk = torch.empty_like(k)
        dv = torch.empty_like(v)
        bgemm(ds_t, qt, out=dk.view(B, Nk, H, d).permute(0, 2, 1, 3))
        bgemm(p_t, dot, out=dv.view(B, Nk, H, d).permute(0, 2, 1, 3))
        return dq, dk, dv, None, None, None


class FlashAttentionFn(Function):
    """The same op without probabilities in HBM (d == 128, bf16 or fp16: the Llama self-attention of the fine-tune step): forward =
    haff_attention_lse_bf16 / _f16 (flash kernel + per-row log-sum-exp), backward = haff_attention_bwd_bf16 / _f16 (recomputes P per
    64 x 64 block; dq / dk / dv in one launch, no transposes, no atomics)."""

    @staticmethod
    def forward(ctx, q, k, v, H, scale_, causal):
        lib = load_library()
        q, k, v = q.contiguous(), k.contiguous(), v.contiguous()
        B, Nq, HD = q.shape
        Nk = k.shape[1]
        d = HD // H
        out = torch.empty_like(q)
        lse = torch.empty((B, H, Nq), dtype=torch.float32, device=q.device)
        check(_fn16(lib, "haff_attention_lse_bf16", q.dtype)(q.data_ptr(), Nq * HD, d, HD, k.data_ptr(), Nk * HD, d, HD, v.data_ptr(), Nk * HD, d, HD,
                                          out.data_ptr(), Nq * HD, d, HD, B, H, Nq, Nk, d, float(scale_), 1 if causal else 0,
                                          Nk - Nq, lse.data_ptr(), _s()), "haff_attention_lse_bf16")
        ctx.save_for_backward(q, k, v, out, lse)
        ctx.cfg = (H, float(scale_), bool(causal))
        return out

    @staticmethod
    def backward(ctx, do):
        lib = load_library()
        q, k, v, out, lse = ctx.saved_tensors
        H, scale_, causal = ctx.cfg
        do = do.contiguous()
        B, Nq, HD = q.shape
        Nk = k.shape[1]
        d = HD // H
        dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
        n_ws = (B * H * Nq + 3) // 4 * 4 + B * H * ((Nq + 63) // 64) * 64 * d   # delta, then the 16-byte aligned fp32 dq sums (haff_hip.h)
        ws = torch.empty((n_ws,), dtype=torch.float32, device=q.device)
        check(_fn16(lib, "haff_attention_bwd_bf16", q.dtype)(q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), do.data_ptr(), lse.data_ptr(),
                                          dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), ws.data_ptr(), n_ws, HD, B, H, Nq, Nk, d,
                                          scale_, 1 if causal else 0, Nk - Nq, _s()), "haff_attention_bwd_bf16")
        return dq, dk, dv, None, None, None


FLASH_TRAINING_ATTENTION = True   # False: every attention of the fine-tune step takes the materialised form (A/B, tests)


def attention(q, k, v, H, scale_, causal):
    """softmax(scale * q k^T [+ causal]) v for token-major q [B,Nq,H*d], k / v [B,Nk,H*d] under autograd."""
    if (FLASH_TRAINING_ATTENTION and q.dtype in HALF and q.shape[2] // H == 128 and (not causal or k.shape[1] >= q.shape[1])
            and (q.shape[2] % 8) == 0):
        return FlashAttentionFn.apply(q, k, v, H, scale_, causal)
    return AttentionFn.apply(q, k, v, H, scale_, causal)


# ------------------------------------------------------------------------------------------------------------------
# Fused LoRA nodes (peft LoRA on the Llama projections, 2Haff/train_ds.py:192-230; --lora_target_modules): q|k|v + RoPE, o_proj /
# down_proj as a Linear with a residual epilogue plus its rank-8 update, gate|up with both updates and SwiGLU (csrc/lora.hip).
# bf16 or fp16 (the *_f16 entry points), rank <= 8 per adapter. An adapter's update is s ((x o keep) A^T) B^T; keep holds the dropout
# mask VALUES: 0 / 1/(1-p) as torch's dropout writes them, or 0 / 1 with the 1/(1-p) folded into s (what train_model passes: one
# Bernoulli launch for the masks, and x * keep is then exact in 16 bits). The rank activations are carried TRANSPOSED, 8 rows per
# adapter ([8 n][Mp], Mp = roundup(M, 16)): they come out of the weight-streaming product with the roles swapped, the stacked A as
# its "activation rows" and the token rows as its "weights", and dA / dB are contractions over the rows (haff_lora_tn), so
# backward needs no transposed copy of an operand. The helpers below are the one statement of each step the nodes share; a
# tensor a node does not have (no mask) goes into save_for_backward as None.
# ------------------------------------------------------------------------------------------------------------------
def _adapter_inputs(x, keep, n):
    """The inputs of n adapters on x. keep: None, one mask for every adapter, or one per adapter (peft gives each adapted Linear its
    own lora_dropout module, train_ds.py:218-230) -> (the n dropped inputs x o keep, the n masks (None: no dropout), per_adapter).
    Adapters that share their input share ONE product: the n entries are then the same tensor."""
    if isinstance(keep, (tuple, list)):
        assert len(keep) == n
        return [x if m is None else _mul(x, m) for m in keep], list(keep), True
    return [x if keep is None else _mul(x, keep)] * n, [keep] * n, False


def _stack_adapters(pairs, K, N, dtype, dev):
    """(A [r][K], B [N][r]) per adapter slot, (None, None) for an adapter that is no target -> (A stack [8 n][K], B stack [n][N][8],
    r, which slots are present): every adapter padded to rank 8 with zeros, an absent one all zero. All present at rank 8 (the
    default) takes no padded copy."""
    n = len(pairs)
    on = [a is not None for a, _ in pairs]
    r = next(a.shape[0] for a, _ in pairs if a is not None)
    if all(on) and r == 8:
        if n == 1:
            return pairs[0][0].contiguous(), pairs[0][1].contiguous().unsqueeze(0), r, on
        return torch.cat([a for a, _ in pairs], 0), torch.stack([b for _, b in pairs], 0), r, on
    a_s = torch.zeros((8 * n, K), dtype=dtype, device=dev)
    b_s = torch.zeros((n, N, 8), dtype=dtype, device=dev)
    for i, (a, b) in enumerate(pairs):
        if on[i]:
            a_s[8 * i:8 * i + r] = a
            b_s[i, :, :r] = b
    return a_s, b_s, r, on


def _rank_rows(M, rows, dtype, dev, all_written=True):
    """[rows][Mp] for transposed rank activations: Mp = roundup(M, 16). The pad columns, and rows the caller will not write, are
    zero (finite for the row contractions); torch.empty only where every element gets written."""
    Mp = (M + 15) // 16 * 16
    return (torch.empty if Mp == M and all_written else torch.zeros)((rows, Mp), dtype=dtype, device=dev)


def _forward_ranks(a_s, xds, on, per_adapter):
    """t^T [8 n][Mp] = A_stack . (x o keep)^T: ONE product over all rank rows when the adapters share their input (an absent
    adapter's zero rows of A give zero rows), else one product per present adapter from ITS dropped input."""
    M = xds[0].shape[0]
    tT = _rank_rows(M, a_s.shape[0], a_s.dtype, a_s.device, not per_adapter or all(on))
    if per_adapter:
        for i in range(len(on)):
            if on[i]:
                ops.linear(a_s[8 * i:8 * i + 8], xds[i], out=tT[8 * i:8 * i + 8, :M])
    else:
        ops.linear(a_s, xds[0], out=tT[:, :M])
    return tT


def _lora_tn(sT, big, out, transposed, scale_):
    """out = scale * sT[:, :M] . big, the contraction over the M rows of csrc/lora.hip: sT [R][Mp] (R = 8 or 16, zero padding),
    big [M][n], out [j][n] or, transposed, [n][j] (j <= R rows of sT wanted). The only caller of haff_lora_tn."""
    R, (M, n) = sT.shape[0], big.shape
    ws = _f32_workspace("haff_lora_tn_workspace_elems", big.device, M, R, n)
    _call16("haff_lora_tn", big.dtype, sT.data_ptr(), sT.stride(0), R, big.data_ptr(), big.stride(0), M, n, ws.data_ptr(), ws.numel(),
            out.data_ptr(), out.stride(0), 1 if out.dtype == torch.float32 else 0, 1 if transposed else 0,
            out.shape[1 if transposed else 0], scale_)
    return out


def _lora_dx(dtT, a_s, masks, per_adapter, dx, scale_):
    """dx += scale * sum over the adapter slots of keep_i o (dt_i . A_i), dtT [8 n][Mp] and A stack [8 n][K] with n = 2 or 3 slots.
    The one choice among the entry points: haff_lora_dx3 for three slots (one mask for all travels as keep_q alone), haff_lora_dx2
    for two slots with a mask each, haff_lora_dx for two slots with one mask or none."""
    M, K = dx.shape
    ptrs = [0 if m is None else m.data_ptr() for m in masks]
    if a_s.shape[0] == 24:
        name, ptrs = "haff_lora_dx3", ptrs if per_adapter else [ptrs[0], 0, 0]
    elif per_adapter:
        name = "haff_lora_dx2"
    else:
        name, ptrs = "haff_lora_dx", ptrs[:1]
    _call16(name, dx.dtype, dtT.data_ptr(), dtT.stride(0), a_s.data_ptr(), K, *ptrs, K, dx.data_ptr(), dx.stride(0), 1, M, K, scale_)


class LoraQKVRopeFn(Function):
    """The adapted q | k | v projection of one Llama layer with RoPE, as ONE autograd node (rotate-half RoPE of transformers'
    LlamaAttention, head dim 128):

        q = rope(x Wq^T + s (xd_q Aq^T) Bq^T),  k = rope(x Wk^T + s (xd_k Ak^T) Bk^T),  v = x Wv^T + s (xd_v Av^T) Bv^T

    Any adapter may be None (not a target): its rank rows are zero and it gets no gradient. keep: None, one mask for all, or one
    per adapter in the slots' order (q, v[, k]). The rank-8 updates ride in one pass over q|k|v together with RoPE; d(qkv) is
    assembled in one pass, without autograd's slice adjoints.

    Slots and launches. q and v adapted, k not (the default targets): the two-slot kernels (haff_lora_qkv_rope_fwd, t^T of 16 rows
    q 0-7 / v 8-15, haff_lora_dx / _dx2). Any other subset: three slots (haff_lora_qkv3_rope_fwd, 24 rows, k in 16-23,
    haff_lora_dx3). Adapters that share one input get one rank product over all their rows, and the two slots then one R = 16
    contraction for both dA; per-adapter masks get one product and one R = 8 contraction per adapter; three slots always contract
    per present adapter. The two slots' dA fills all 8 rank rows of a [16][K] buffer, three slots write r rows each."""

    @staticmethod
    def forward(ctx, x, wqkv, wqkv_t, aq, bq, av, bv, ak, bk, cos_sin, T, heads, scale_, keep):
        M, K = x.shape
        fw = ctx.frozen = frozen(wqkv, wqkv_t)
        H = fw.shape[0] // 3
        dev = x.device
        x = x.contiguous()
        qkv = ops.linear(x, fw.w())
        pairs = [(aq, bq), (av, bv), (ak, bk)]
        if aq is not None and av is not None and ak is None:
            pairs = pairs[:2]
        n = len(pairs)
        xds, masks, per_adapter = _adapter_inputs(x, keep[:n] if isinstance(keep, (tuple, list)) else keep, n)
        a_s, b_s, r, on = _stack_adapters(pairs, K, H, x.dtype, dev)
        tT = _forward_ranks(a_s, xds, on, per_adapter)
        q, k, v = (torch.empty((M, H), dtype=x.dtype, device=dev) for _ in range(3))
        name = "haff_lora_qkv_rope_fwd" if n == 2 else "haff_lora_qkv3_rope_fwd"
        _call16(name, x.dtype, qkv.data_ptr(), qkv.stride(0), tT.data_ptr(), tT.stride(0), *[b.data_ptr() for b in b_s], 8, cos_sin.data_ptr(),
                q.data_ptr(), k.data_ptr(), v.data_ptr(), H, M, H, H // heads, int(T), float(scale_))
        ctx.save_for_backward(a_s, b_s, tT, cos_sin, *xds, *masks)
        ctx.cfg = (int(T), heads, float(scale_), r, on, per_adapter)
        return q, k, v

    @staticmethod
    def backward(ctx, dq, dk, dv):
        a_s, b_s, tT, cos_sin, *rest = ctx.saved_tensors
        T, heads, scale_, r, on, per_adapter = ctx.cfg
        n, H = b_s.shape[0], b_s.shape[1]
        xds, masks = rest[:n], rest[n:]
        M, K = xds[0].shape
        dev, dt_ = xds[0].device, xds[0].dtype
        dq, dk, dv = dq.contiguous(), dk.contiguous(), dv.contiguous()
        dqkv = torch.empty((M, 3 * H), dtype=dt_, device=dev)
        _call16("haff_lora_qkv_rope_bwd", dt_, dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), H, cos_sin.data_ptr(), dqkv.data_ptr(), 3 * H, M, H,
                H // heads, T)
        cols = [dqkv[:, :H], dqkv[:, 2 * H:], dqkv[:, H:2 * H]]   # q, v, k: the adapters' order in t^T
        rows = [slice(8 * i, 8 * i + 8) for i in range(n)]
        b_t = b_s.transpose(1, 2).contiguous()                     # [n][8][H]
        dtT = _rank_rows(M, 8 * n, dt_, dev, all(on))

        def dt_rows(i):   # dt_i^T [8][M] = B_i^T . d(q|v|k)^T: the weight-streaming product again, the gradient rows as its "weights"
            ops.linear(b_t[i], cols[i], out=dtT[rows[i], :M])

        def d_b(i):
            return _lora_tn(tT[rows[i]], cols[i], torch.empty((H, r), dtype=dt_, device=dev), True, scale_)

        da, db = [None] * 3, [None] * 3
        if n == 2:
            dt_rows(0)
            dt_rows(1)
            db[0], db[1] = d_b(0), d_b(1)
            da2 = torch.empty((16, K), dtype=dt_, device=dev)
            if per_adapter:   # each adapter's dA against ITS dropped input
                for i in range(2):
                    _lora_tn(dtT[rows[i]], xds[i], da2[rows[i]], False, scale_)
            else:
                _lora_tn(dtT, xds[0], da2, False, scale_)
            da[0], da[1] = da2[0:r], da2[8:8 + r]
        else:
            for i in range(3):
                if on[i]:
                    dt_rows(i)
                    db[i] = d_b(i)
                    da[i] = _lora_tn(dtT[rows[i]], xds[i], torch.empty((r, K), dtype=dt_, device=dev), False, scale_)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ops.linear(dqkv, ctx.frozen.w_t())
            _lora_dx(dtT, a_s, masks, per_adapter, dx, scale_)
        return dx, None, None, da[0], db[0], da[1], db[1], da[2], db[2], None, None, None, None, None


def lora_qkv_rope_supported(x, wqkv, aq, heads):
    H = wqkv.shape[0] // 3
    return (x.dtype in HALF and wqkv.dtype == x.dtype and H % heads == 0 and H // heads == 128 and aq.shape[0] <= 8 and x.shape[1] % 128 == 0
            and x.shape[0] >= 16)


FUSED_LORA_QKV = True   # False: the adapters run as separate LinearFn / scale / add / rope nodes (A/B, tests)


def lora_qkv3_rope(x, wqkv, wqkv_t, aq, bq, av, bv, ak, bk, cos_sin, T, heads, scale_, keep=None):
    return LoraQKVRopeFn.apply(x, wqkv, wqkv_t, aq, bq, av, bv, ak, bk, cos_sin, T, heads, scale_, keep)


def lora_qkv_rope(x, wqkv, wqkv_t, aq, bq, av, bv, cos_sin, T, heads, scale_, keep=None):
    """The q and v adapters alone (peft's default targets)."""
    return lora_qkv3_rope(x, wqkv, wqkv_t, aq, bq, av, bv, None, None, cos_sin, T, heads, scale_, keep)


class LoraLinearFn(Function):
    """An adapted Llama Linear with a residual epilogue (o_proj, down_proj): y = x W^T + resid + s ((x o keep) A^T) B^T.
    The frozen product carries the residual as today; one haff_lora_out pass adds the rank-8 update to its rows."""

    @staticmethod
    def forward(ctx, x, w, w_t, resid, a, b, scale_, keep):
        M, K = x.shape
        fw = ctx.frozen = frozen(w, w_t)
        N = fw.shape[0]
        x = x.contiguous()
        y = ops.linear(x, fw.w(), resid=resid)
        (xd,), (keep,), _ = _adapter_inputs(x, keep, 1)
        a8, b8, r, on = _stack_adapters([(a, b)], K, N, x.dtype, x.device)
        tT = _forward_ranks(a8, [xd], on, False)
        _call16("haff_lora_out", x.dtype, tT.data_ptr(), tT.stride(0), b8.data_ptr(), y.data_ptr(), y.stride(0), M, N, float(scale_))
        ctx.save_for_backward(xd, a8, b8[0], tT, keep)
        ctx.cfg = (float(scale_), r, resid is not None)
        return y

    @staticmethod
    def backward(ctx, dy):
        xd, a8, b8, tT, keep = ctx.saved_tensors
        scale_, r, has_resid = ctx.cfg
        M, K = xd.shape
        N = b8.shape[0]
        dev, dt_ = xd.device, xd.dtype
        dy = dy.contiguous()
        # haff_lora_dx reads 16 rank rows (two adapter slots) of dt^T and A: this adapter's in rows 0-7, rows 8-15 zero
        dtT = torch.zeros((16, tT.shape[1]), dtype=dt_, device=dev)
        ops.linear(b8.t().contiguous(), dy, out=dtT[0:8, :M])
        db = _lora_tn(tT, dy, torch.empty((N, r), dtype=dt_, device=dev), True, scale_)
        da = _lora_tn(dtT[0:8], xd, torch.empty((r, K), dtype=dt_, device=dev), False, scale_)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ops.linear(dy, ctx.frozen.w_t())
            _lora_dx(dtT, torch.cat([a8, torch.zeros_like(a8)], 0), [keep], False, dx, scale_)
        return dx, None, None, (dy if has_resid else None), da, db, None, None


def lora_linear(x, w, w_t, resid, a, b, scale_, keep=None):
    return LoraLinearFn.apply(x, w, w_t, resid, a, b, scale_, keep)


class LoraGateUpSwigluFn(Function):
    """The adapted gate | up product with SwiGLU: gu' = x Wgu^T + s ((x o keep_g) Ag^T) Bg^T (gate columns) and
    + s ((x o keep_u) Au^T) Bu^T (up columns) in the interleaved [gate x16 | up x16] layout, y = silu(g') * u'. Either adapter may
    be None. keep: None, one mask for both, or a pair (gate, up). gu' stays for the SwiGLU adjoint, as SwigluFn keeps gu."""

    @staticmethod
    def forward(ctx, x, wgu, wgu_t, ag, bg, au, bu, scale_, keep):
        M, K = x.shape
        fw = ctx.frozen = frozen(wgu, wgu_t)
        F = fw.shape[0] // 2
        x = x.contiguous()
        gu = ops.linear(x, fw.w())
        xds, masks, per_adapter = _adapter_inputs(x, keep, 2)
        a2, b2, r, on = _stack_adapters([(ag, bg), (au, bu)], K, F, x.dtype, x.device)
        tT = _forward_ranks(a2, xds, on, per_adapter)
        y = torch.empty((M, F), dtype=x.dtype, device=x.device)
        _call16("haff_lora_gu_swiglu", x.dtype, tT.data_ptr(), tT.stride(0), b2[0].data_ptr(), b2[1].data_ptr(), gu.data_ptr(), gu.stride(0),
                y.data_ptr(), F, M, F, float(scale_))
        ctx.save_for_backward(gu, a2, b2, tT, *xds, *masks)
        ctx.cfg = (float(scale_), r, on, per_adapter)
        return y

    @staticmethod
    def backward(ctx, dy):
        gu, a2, b2, tT, xg, xu, *masks = ctx.saved_tensors
        scale_, r, on, per_adapter = ctx.cfg
        M, K = xg.shape
        F = b2.shape[1]
        dev, dt_ = xg.device, xg.dtype
        dy = dy.contiguous()
        dgu = torch.empty_like(gu)
        _call("haff_swiglu_bwd", gu.data_ptr(), dy.data_ptr(), dgu.data_ptr(), M, F, _dt(gu))
        # dt^T [16][M] = Bblk^T . dgu'^T in one weight-streaming launch: Bblk^T [16][2F] holds Bg^T on the gate columns (rows 0-7)
        # and Bu^T on the up columns (rows 8-15), zeros elsewhere
        blk = torch.zeros((16, F // 16, 2, 16), dtype=dt_, device=dev)
        blk[0:8, :, 0, :] = b2[0].t().reshape(8, F // 16, 16)
        blk[8:16, :, 1, :] = b2[1].t().reshape(8, F // 16, 16)
        dtT = _rank_rows(M, 16, dt_, dev)
        ops.linear(blk.view(16, 2 * F), dgu, out=dtT[:, :M])
        dag = dbg = dau = dbu = None
        db_all = _lora_tn(tT, dgu, torch.empty((2 * F, 16), dtype=dt_, device=dev), True, scale_)
        db_all = db_all.view(F // 16, 2, 16, 16)
        if on[0]:
            dbg = db_all[:, 0, :, 0:r].reshape(F, r)
            dag = _lora_tn(dtT[0:8], xg, torch.empty((r, K), dtype=dt_, device=dev), False, scale_)
        if on[1]:
            dbu = db_all[:, 1, :, 8:8 + r].reshape(F, r)
            dau = _lora_tn(dtT[8:16], xu, torch.empty((r, K), dtype=dt_, device=dev), False, scale_)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = ops.linear(dgu, ctx.frozen.w_t())
            _lora_dx(dtT, a2, masks, per_adapter, dx, scale_)
        return dx, None, None, dag, dbg, dau, dbu, None, None


def lora_gate_up_swiglu(x, wgu, wgu_t, ag, bg, au, bu, scale_, keep=None):
    return LoraGateUpSwigluFn.apply(x, wgu, wgu_t, ag, bg, au, bu, scale_, keep)


def lora_fused_supported(x, w, a):
    """The fused adapter nodes' shapes: 16-bit operands, K % 128 == 0 (haff_lora_dx), N % 16 == 0, rank <= 8, M >= 16."""
    return (x.dtype in HALF and w.dtype == x.dtype and x.shape[1] % 128 == 0 and w.shape[0] % 16 == 0 and a.shape[0] <= 8
            and x.shape[0] >= 16)


FUSED_LORA_OUT = True      # False: o_proj / down_proj adapters as LinearFn / scale / add nodes (A/B, tests)
FUSED_LORA_GATE_UP = True  # False: gate / up adapters as LinearFn nodes added into gu before SwigluFn (A/B, tests)


class BgemmFn(Function):
    """c[z] = a[z] @ b[z].T for a [Z,M,K], b [Z,N,K]."""

    @staticmethod
    def forward(ctx, a, b):
        a, b = a.contiguous(), b.contiguous()
        ctx.save_for_backward(a, b)
        return bgemm(a.unsqueeze(1), b.unsqueeze(1), out_dtype=a.dtype).squeeze(1)

    @staticmethod
    def backward(ctx, dc):
        a, b = ctx.saved_tensors
        dc = dc.contiguous()
        Z, M, K = a.shape
        N = b.shape[1]
        Np, Mp = _pad8(N), _pad8(M)
        bt = transpose(b, Rp=Np).view(Z, 1, K, Np)
        dcp = dc
        if Np != N:
            dcp = torch.zeros((Z, M, Np), dtype=dc.dtype, device=dc.device)
            dcp[..., :N] = dc
        da = bgemm(dcp.unsqueeze(1), bt, out_dtype=a.dtype).squeeze(1)          # [Z,M,K]
        dct = transpose(dc, Rp=Mp).view(Z, 1, N, Mp)
        at = transpose(a, Rp=Mp).view(Z, 1, K, Mp)
        db = bgemm(dct, at, out_dtype=b.dtype).squeeze(1)                       # [Z,N,K]
        return da, db


bmm_nt = BgemmFn.apply


class EmbedFn(Function):
    @staticmethod
    def forward(ctx, weight, ids):
        ctx.save_for_backward(ids)
        ctx.shape = weight.shape
        ctx.wdtype = weight.dtype
        safe = ids.clamp(min=0)
        return weight.index_select(0, safe.reshape(-1)).view(*ids.shape, weight.shape[1])

    @staticmethod
    def backward(ctx, dy):
        (ids,) = ctx.saved_tensors
        dy = dy.contiguous()
        acc = torch.zeros(ctx.shape, dtype=torch.float32, device=dy.device)
        flat = ids.reshape(-1).contiguous()
        if ORDERED_REDUCTIONS:   # rows that share an id are added in row order (stable sort on the device: no host read)
            sorted_ids, order = torch.sort(flat, stable=True)
            _call("haff_scatter_add_rows_sorted", sorted_ids.data_ptr(), order.data_ptr(), dy.data_ptr(), acc.data_ptr(), flat.numel(),
                  ctx.shape[1], _dt(dy))
        else:
            _call("haff_scatter_add_rows", flat.data_ptr(), dy.data_ptr(), acc.data_ptr(), flat.numel(), ctx.shape[1], _dt(dy))
        return acc.to(ctx.wdtype), None


embed = EmbedFn.apply


class CrossEntropyFn(Function):
    """mean over rows with label >= 0 of (logsumexp(logits) - logits[label])  (CrossEntropyLoss, ignore_index=-100)."""

    @staticmethod
    def forward(ctx, logits, labels, n_valid=None):
        logits = logits.contiguous()
        labels = labels.contiguous()
        R, V = logits.shape
        if n_valid is None:   # (a host read: callers that know the count — the labels came from the host — pass it)
            n_valid = int((labels >= 0).sum().item())
        n_valid = max(int(n_valid), 1)
        row_loss = torch.empty((R,), dtype=torch.float32, device=logits.device)
        dlogits = torch.empty_like(logits)
        # fp16: the kernel writes softmax - onehot unscaled and the 1 / n_valid joins the upstream (loss-scaled) gradient in backward:
        # softmax / n_valid itself would fall below fp16's subnormals for a 32003-word vocabulary before the loss scale reaches it
        ctx.post = n_valid if logits.dtype == torch.float16 else None
        _call("haff_cross_entropy", logits.data_ptr(), logits.stride(0), labels.data_ptr(), row_loss.data_ptr(), dlogits.data_ptr(), R, V,
              1.0 if ctx.post else 1.0 / n_valid, _dt(logits))
        ctx.save_for_backward(dlogits)
        # sum of R floats / n_valid: reduction of a tiny vector (torch sum as plumbing of a scalar)
        return (row_loss.sum() / n_valid).to(torch.float32)

    @staticmethod
    def backward(ctx, g):
        (dlogits,) = ctx.saved_tensors
        if ctx.post:
            g = g.to(torch.float32) / ctx.post
        return scale_dev(dlogits, g), None, None   # the upstream scalar stays on the device AND in fp32 (no read-back, no bf16 rounding)


def cross_entropy(logits, labels, n_valid=None):
    return CrossEntropyFn.apply(logits, labels, n_valid)


class MaskLossFn(Function):
    """Per-sample [bce_i, dice_i] (LISA.py:16-59) of f32 logits x [n, HW] scaled by wgt[i] against targets t."""

    @staticmethod
    def forward(ctx, x, t, wgts):
        x, t = x.contiguous(), t.contiguous()
        n, hw = x.shape
        stats = torch.zeros((n, 4), dtype=torch.float32, device=x.device)
        if n == 0 or hw == 0:
            ctx.save_for_backward(x, t, stats)
            ctx.wgts = []
            return torch.zeros((n, 2), dtype=torch.float32, device=x.device)
        if ORDERED_REDUCTIONS:
            import ctypes
            # Layout (one convention, stated once — ADVICE r4): the kernel entry writes partials [n_samples][*n_parts][4] for ITS
            # launch. Here every sample is its own launch (n_samples = 1: the per-sample weight is a host scalar), writing the first
            # n_parts rows of its own SLOTS-row slab partials[i]; the reduce walks sample i's parts at group stride SLOTS * 4.
            SLOTS = 256
            partials = torch.empty((n, SLOTS, 4), dtype=torch.float32, device=x.device)
            n_parts = ctypes.c_int(0)
            for i in range(n):  # per-sample weight is a host scalar (taxonomy one-hot sums)
                _call("haff_mask_loss_stats_partials", x[i].data_ptr(), t[i].data_ptr(), partials[i].data_ptr(), 1, hw, float(wgts[i]),
                      ctypes.byref(n_parts))
                assert 0 < n_parts.value <= SLOTS, n_parts.value
            # stats[i][k] = sum over the parts of sample i, in index order (one launch for all samples)
            _reduce_partials(partials, stats, 4 * n, n_parts.value, 4, 4, SLOTS * 4, False)
        else:
            for i in range(n):
                _call("haff_mask_loss_stats", x[i].data_ptr(), t[i].data_ptr(), stats[i].data_ptr(), 1, hw, float(wgts[i]))
        ctx.save_for_backward(x, t, stats)
        ctx.wgts = [float(w) for w in wgts]
        # four sums per sample -> {bce, dice}: a handful of n-element device ops (scalar plumbing; a host round trip here
        # would drain the launch queue once per frame and hand)
        bce = stats[:, 0] / hw
        num = 2 * stats[:, 1] / 1000 + 1e-6
        den = stats[:, 2] / 1000 + stats[:, 3] / 1000 + 1e-6
        return torch.stack([bce, 1 - num / den], dim=1)

    @staticmethod
    def backward(ctx, g):
        x, t, stats = ctx.saved_tensors
        n, hw = x.shape
        coef = g.to(torch.float32).contiguous()   # [n, 2] upstream gradients of {bce, dice}: read by the kernel, not by the host
        dx = torch.empty_like(x)
        if n == 0 or hw == 0:
            return dx, None, None
        for i in range(n):
            _call("haff_mask_loss_grad_dev", x[i].data_ptr(), t[i].data_ptr(), stats[i].data_ptr(), dx[i].data_ptr(), 1, hw, ctx.wgts[i],
                  coef[i].data_ptr())
        return dx, None, None


mask_losses = MaskLossFn.apply


class BilinearFn(Function):
    @staticmethod
    def forward(ctx, x, crop_hw, out_hw):
        x = x.contiguous()
        ctx.geom = (tuple(x.shape), tuple(int(v) for v in crop_hw), tuple(int(v) for v in out_hw))
        return ops.resize_bilinear(x, crop_hw, out_hw)

    @staticmethod
    def backward(ctx, dy):
        (N, Hs, Ws), (Hc, Wc), (Ho, Wo) = ctx.geom
        dy = dy.contiguous()
        dx = torch.zeros((N, Hs, Ws), dtype=torch.float32, device=dy.device)
        _call("haff_resize_bilinear_bwd", dy.data_ptr(), dx.data_ptr(), N, Hs, Ws, Hc, Wc, Ho, Wo)
        return dx, None, None


resize_bilinear = BilinearFn.apply


class CastFn(Function):
    """dtype change (bf16 / fp16 <-> f32) — a copy, kept as a Function so gradients come back in the source dtype."""

    @staticmethod
    def forward(ctx, x, dtype):
        ctx.src = x.dtype
        return x.to(dtype)

    @staticmethod
    def backward(ctx, dy):
        return dy.to(ctx.src), None


cast = CastFn.apply


class TaxonomyCEFn(Function):
    """sum over rows of CrossEntropyLoss(softmax(z), soft target) — LISA.py:414-417 (input is already soft-maxed)."""

    @staticmethod
    def forward(ctx, z, t):
        z, t = z.contiguous(), t.contiguous().float()
        R, C = z.shape
        loss = torch.empty((R,), dtype=torch.float32, device=z.device)
        dz = torch.empty_like(z)
        probs = torch.empty_like(z)
        _call("haff_taxonomy_ce", z.data_ptr(), t.data_ptr(), probs.data_ptr(), loss.data_ptr(), dz.data_ptr(), R, C)
        ctx.save_for_backward(dz)
        ctx.mark_non_differentiable(probs)
        return loss, probs

    @staticmethod
    def backward(ctx, g, _gp):
        (dz,) = ctx.saved_tensors
        return scale_dev(dz, g, per_row=True), None   # per-row upstream scalar, applied on the device in fp32


taxonomy_ce = TaxonomyCEFn.apply
