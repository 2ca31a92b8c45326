"""fp16 fine-tuning kernels (the f16 instances of every kernel the fine-tune step launches) against torch fp32 on the same
f16-representable inputs, at production widths (Llama 7B / 13B: H 4096 / 5120, head dim 128, ffn 11008 / 13824, vocab 32003) and
at odd sizes; fp16's edges (values near 65504, subnormal gradients, one inf / NaN element); the AdamW step's f16 copy and its
skip on a non-finite gradient norm; and the refusal of dtype codes without an instance."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

F16 = torch.float16


def _f16(shape, scale=1.0, seed=0, dev="cuda:0"):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(F16).to(dev)


def _rel(got, ref):
    return ((got.float().cpu() - ref.float().cpu()).norm() / (ref.float().cpu().norm() + 1e-30)).item()


def _ulps16(got, ref):
    """max distance in f16 units in the last place between an f16 result and the f16 rounding of an f32 reference"""
    a = got.cpu().view(torch.int16).int()
    b = ref.to(F16).cpu().view(torch.int16).int()
    a = torch.where(a < 0, -32768 - a, a)
    b = torch.where(b < 0, -32768 - b, b)
    return int((a - b).abs().max())


# ---- DISPATCH_T: codes without an instance are refused, nothing runs -------------------------------------------------------------
def test_unknown_dtype_codes_are_refused(dev):
    import haff  # noqa: F401
    from haff.lib import load_library
    lib = load_library()
    x = torch.zeros(1024, device=dev)
    y = torch.full((1024,), 7.0, device=dev)
    for code in (2, 4, -1, 9):
        assert lib.haff_act_fwd(x.data_ptr(), y.data_ptr(), 1024, 3, code, None) == -1
        assert lib.haff_axpby(x.data_ptr(), 0, y.data_ptr(), 1024, 1.0, 0.0, code, None) == -1
        assert lib.haff_mul(x.data_ptr(), x.data_ptr(), y.data_ptr(), 1024, code, None) == -1
        n = ctypes.c_int(0)
        assert lib.haff_sumsq_partials(x.data_ptr(), y.data_ptr(), 1024, code, ctypes.byref(n), None) == -1
        assert lib.haff_norm_bwd(x.data_ptr(), x.data_ptr(), x.data_ptr(), y.data_ptr(), 0, 4, 256, 1e-6, 1, code, None) == -1
        assert lib.haff_adamw_step(x.data_ptr(), x.data_ptr(), x.data_ptr(), x.data_ptr(), 0, 1024, 1e-3, 0.9, 0.95, 1e-8, 0.0, 1,
                                   1.0, code, -1, None) == -1
    torch.cuda.synchronize()
    assert torch.all(y == 7.0)   # no launch wrote anything


# ---- elementwise f16 kernels: exact where a CPU restatement is exact --------------------------------------------------------------
@pytest.mark.parametrize("F", [11008, 13824, 48])
def test_swiglu_and_mul_f16(dev, F):
    from haff import autograd as A
    M = 37
    gu = _f16((M, 2 * F), 2.0, 1).requires_grad_(True)
    y = A.swiglu(gu)
    g = gu.detach().float().cpu().view(M, F // 16, 2, 16)
    gate, up = g[:, :, 0].reshape(M, F), g[:, :, 1].reshape(M, F)
    ref = torch.nn.functional.silu(gate) * up
    assert _ulps16(y.detach(), ref) <= 1
    dy = _f16((M, F), 1.0, 2)
    y.backward(dy)
    gr, ur = gate.clone().requires_grad_(True), up.clone().requires_grad_(True)
    (torch.nn.functional.silu(gr) * ur).backward(dy.float().cpu())
    dgu = gu.grad.float().cpu().view(M, F // 16, 2, 16)
    assert _ulps16(dgu[:, :, 0].reshape(M, F).to(F16), gr.grad) <= 2
    assert _ulps16(dgu[:, :, 1].reshape(M, F).to(F16), ur.grad) <= 1
    a, b = _f16((M, F), 3.0, 3), _f16((M, F), 3.0, 4)
    assert torch.equal(A._mul(a, b).cpu(), (a.float() * b.float()).to(F16).cpu())        # one rounding of an exact product


@pytest.mark.parametrize("R,C", [(4096, 4096), (5120, 4000), (33, 77)])
def test_transpose_f16_is_exact(dev, R, C):
    from haff import autograd as A
    x = _f16((R, C), 1.0, 5)
    t = A.transpose(x, Rp=(R + 7) // 8 * 8)[0]
    assert torch.equal(t[:, :R].cpu(), x.t().cpu()) and not t[:, R:].any()


def test_rope_act_axpby_scale_f16(dev):
    from haff import autograd as A
    from haff.lib import check, load_library
    lib = load_library()
    T_, H, d = 40, 32, 128
    x = _f16((2 * T_, H * d), 1.0, 6)
    pos = torch.arange(T_, dtype=torch.float32)[:, None]
    inv = 1.0 / (10000 ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
    ang = pos * inv[None]
    cs = torch.cat([ang.cos(), ang.sin()], 1).contiguous()
    y = A.rope(x, cs.to(dev), T_, H, d)
    xf = x.float().cpu().view(2, T_, H, d)
    c, s = ang.cos()[None, :, None], ang.sin()[None, :, None]
    x1, x2 = xf[..., :d // 2], xf[..., d // 2:]
    ref = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).view(2 * T_, H * d)
    assert _ulps16(y, ref) <= 1
    for code, fn in ((1, lambda v: torch.nn.functional.gelu(v)), (3, torch.relu), (4, torch.nn.functional.silu)):
        z = _f16((1000, 257), 3.0, 7)
        out = torch.empty_like(z)
        check(lib.haff_act_fwd(z.data_ptr(), out.data_ptr(), z.numel(), code, 3, A._s()), "act")
        ref = fn(z.float().cpu())   # the kernels' erf / exp are the device's fast forms (as in the bf16 instance): a few ulps
        assert ((out.float().cpu() - ref).abs() <= 2e-3 * ref.abs() + 1e-6).all(), code
    a, b = _f16((5000,), 100.0, 8), _f16((5000,), 100.0, 9)
    assert _ulps16(A.axpby(a, b, 0.5, -2.0), 0.5 * a.float().cpu() - 2.0 * b.float().cpu()) <= 1
    al = torch.tensor([3.0], device=dev)
    assert _ulps16(A.scale_dev(a, al), 3.0 * a.float().cpu()) <= 1


# ---- norm adjoints (one-pass 4096 / 5120 rows and the generic kernel), column sums, norms of f16 gradients ------------------------
@pytest.mark.parametrize("C", [4096, 5120, 200])
def test_rmsnorm_and_layernorm_adjoints_f16(dev, C):
    from haff import autograd as A
    rows = 70
    x = _f16((rows, C), 1.0, 10)
    w = (1 + 0.1 * torch.randn(C, generator=torch.Generator().manual_seed(11))).to(dev)
    b = torch.zeros(C, device=dev)
    dy = _f16((rows, C), 1.0, 12)
    for kind in ("rms", "ln", "resid"):
        xg = x.clone().requires_grad_(True)
        xr = x.float().cpu().requires_grad_(True)
        if kind == "rms":
            A.rmsnorm(xg, w, 1e-6).backward(dy)
            (xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + 1e-6) * w.cpu()).backward(dy.float().cpu())
        elif kind == "ln":
            A.layernorm(xg, w, b, 1e-5).backward(dy)
            torch.nn.functional.layer_norm(xr, (C,), w.cpu(), b.cpu(), 1e-5).backward(dy.float().cpu())
        else:
            res = _f16((rows, C), 1.0, 13)
            xs, h = A.resid_rmsnorm(xg, w, 1e-6)
            torch.autograd.backward([xs, h], [res, dy])
            x_, h_ = xr, xr * torch.rsqrt(xr.pow(2).mean(-1, keepdim=True) + 1e-6) * w.cpu()
            torch.autograd.backward([x_, h_], [res.float().cpu(), dy.float().cpu()])
        assert _rel(xg.grad, xr.grad) < 2e-3, kind


def test_colsum_sumsq_scatter_f16(dev):
    from haff import autograd as A
    from haff import train_ops as T
    for R, C in ((65536, 256), (1000, 4096), (13, 40)):
        x = _f16((R, C), 4.0, 14)
        assert _rel(A.colsum(x), x.float().sum(0)) < 1e-5
    gs = [_f16((4096, 8), 1.0, 15), _f16((5000,), 300.0, 16), _f16((77,), 1.0, 17)]
    norm = T.grad_norm(gs)
    ref = torch.sqrt(sum((g.double() ** 2).sum() for g in gs))
    assert abs(norm.item() - ref.item()) <= 1e-5 * ref.item()
    ids = torch.tensor([3, 1, 3, -1, 0, 3], device=dev)
    dy = _f16((6, 4096), 1.0, 18)
    wgt = torch.zeros((5, 4096), dtype=F16, device=dev, requires_grad=True)
    A.embed(wgt, ids.view(1, 6)).backward(dy.view(1, 6, 4096))
    ref = torch.zeros((5, 4096))
    for r, i in enumerate(ids.tolist()):
        if i >= 0:
            ref[i] += dy[r].float().cpu()
    assert torch.equal(wgt.grad.cpu(), ref.to(F16))


def test_cross_entropy_f16_vocab_32003(dev):
    from haff import autograd as A
    R, V = 300, 32003
    logits = _f16((R, V), 4.0, 19)
    logits[5, 17] = 65504.0                       # fp16's largest value: lse stays f32
    logits[6] = -60000.0
    labels = torch.randint(0, V, (R,), generator=torch.Generator().manual_seed(20)).to(dev)
    labels[::7] = -100
    lg = logits.clone().requires_grad_(True)
    loss = A.cross_entropy(lg, labels)
    loss.backward()
    lr = logits.float().cpu().requires_grad_(True)
    ref = torch.nn.functional.cross_entropy(lr, labels.cpu(), ignore_index=-100)
    ref.backward()
    assert abs(loss.item() - ref.item()) <= 1e-5 * max(1.0, abs(ref.item()))
    assert lg.grad.dtype == F16 and torch.isfinite(lg.grad).all()
    assert _rel(lg.grad, lr.grad) < 1e-3


# ---- matrix-core products ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N1,N2", [(2808, 4096, 256), (65536, 256, 256), (1000, 5120, 32), (37, 24, 40)])
def test_gemm_tn_f16(dev, M, N1, N2):
    from haff import autograd as A
    a, b = _f16((M, N1), 1.0, 21), _f16((M, N2), 1.0, 22)
    assert A.gemm_tn_supported(a, b)
    ref = a.float().t() @ b.float()
    for od in (F16, torch.float32):
        out = A.gemm_tn(a, b, out_dtype=od)
        assert out.dtype == od and _rel(out, ref) < (1e-3 if od == F16 else 1e-5)


@pytest.mark.parametrize("Z,M,N,K", [(64, 351, 351, 128), (16, 6, 4096, 32), (3, 37, 45, 24)])
def test_batched_product_f16(dev, Z, M, N, K):
    from haff import autograd as A
    a, w = _f16((Z, 1, M, K), 1.0, 23), _f16((Z, 1, N, K), 1.0, 24)
    ref = a.float() @ w.float().transpose(-1, -2)
    assert _rel(A.bgemm(a, w, out_dtype=torch.float32), ref) < 1e-5
    assert _rel(A.bgemm(a, w), ref) < 1e-3


@pytest.mark.parametrize("H,T,causal", [(32, 351, True), (40, 200, True), (8, 70, False)])
def test_flash_attention_pair_f16(dev, H, T, causal):
    from haff import autograd as A
    B, d = 2, 128
    q, k, v = (_f16((B, T, H * d), 1.0, s).requires_grad_(True) for s in (25, 26, 27))
    o = A.attention(q, k, v, H, d ** -0.5, causal)
    do = _f16((B, T, H * d), 1.0, 28)
    o.backward(do)
    qf, kf, vf = (t.detach().float().view(B, T, H, d).transpose(1, 2).requires_grad_(True) for t in (q, k, v))
    of = torch.nn.functional.scaled_dot_product_attention(qf, kf, vf, is_causal=causal, scale=d ** -0.5)
    of.backward(do.float().view(B, T, H, d).transpose(1, 2))
    back = lambda t: t.transpose(1, 2).reshape(B, T, H * d)   # noqa: E731
    assert _rel(o.detach(), back(of.detach())) < 2e-3
    for got, ref in ((q.grad, qf.grad), (k.grad, kf.grad), (v.grad, vf.grad)):
        assert got.dtype == F16 and _rel(got, back(ref)) < 5e-3


@pytest.mark.parametrize("H,heads,r,two", [(4096, 32, 8, True), (5120, 40, 8, False), (256, 2, 4, True)])
def test_lora_qkv_rope_node_f16(dev, H, heads, r, two):
    """The adapted q|k|v + RoPE node (haff_lora_qkv_rope_fwd/bwd_f16, haff_lora_dx(2)_f16, haff_lora_tn_f16) against torch fp32."""
    from haff import autograd as A
    M, T_ = 2 * 103, 103
    d = H // heads
    x = _f16((M, H), 1.0, 30).requires_grad_(True)
    wqkv = _f16((3 * H, H), H ** -0.5, 31)
    wt = A.transpose(wqkv)[0]
    aq, av = (_f16((r, H), H ** -0.5, s).requires_grad_(True) for s in (32, 33))
    bq, bv = (_f16((H, r), 0.05, s).requires_grad_(True) for s in (34, 35))
    pos = torch.arange(T_, dtype=torch.float32)[:, None]
    ang = pos * (1.0 / (10000 ** (torch.arange(0, d, 2, dtype=torch.float32) / d)))[None]
    cs = torch.cat([ang.cos(), ang.sin()], 1).contiguous()
    g = torch.Generator().manual_seed(36)
    keeps = [(torch.rand((M, H), generator=g) > 0.1).to(F16).to(dev) for _ in range(2 if two else 1)]
    keep = tuple(keeps) if two else keeps[0]
    assert A.lora_qkv_rope_supported(x, wqkv, aq, heads)
    s = 2.0 / 0.9
    q, k, v = A.lora_qkv_rope(x, wqkv, wt, aq, bq, av, bv, cs.to(dev), T_, heads, s, keep)
    dq, dk, dv = (_f16((M, H), 1.0, s_) for s_ in (37, 38, 39))
    torch.autograd.backward([q, k, v], [dq, dk, dv])
    X = x.detach().float().cpu().requires_grad_(True)
    Aq, Av, Bq, Bv = (t.detach().float().cpu().requires_grad_(True) for t in (aq, av, bq, bv))
    Kq, Kv = keeps[0].float().cpu(), keeps[-1].float().cpu()
    W = wqkv.float().cpu()
    qkv = X @ W.t()

    def rope(t):
        t = t.view(2, T_, heads, d)
        c, sn = ang.cos()[None, :, None], ang.sin()[None, :, None]
        t1, t2 = t[..., :d // 2], t[..., d // 2:]
        return torch.cat([t1 * c - t2 * sn, t2 * c + t1 * sn], -1).reshape(M, H)
    Q = rope(qkv[:, :H] + s * ((X * Kq) @ Aq.t()) @ Bq.t())
    Kk = rope(qkv[:, H:2 * H])
    Vv = qkv[:, 2 * H:] + s * ((X * Kv) @ Av.t()) @ Bv.t()
    torch.autograd.backward([Q, Kk, Vv], [dq.float().cpu(), dk.float().cpu(), dv.float().cpu()])
    for got, ref in ((q, Q), (k, Kk), (v, Vv)):
        assert _rel(got.detach(), ref.detach()) < 2e-3
    for got, ref, name in ((x.grad, X.grad, "x"), (aq.grad, Aq.grad, "Aq"), (av.grad, Av.grad, "Av"), (bq.grad, Bq.grad, "Bq"),
                           (bv.grad, Bv.grad, "Bv")):
        assert got.dtype == F16 and _rel(got, ref) < 5e-3, name


# ---- AdamW: the f16 copy, the overflow skip, fp16 gradient edges ------------------------------------------------------------------
def test_adamw_f16_copy_is_f16_rn_of_master(dev):
    from haff import train_ops as T
    p = _f16((100003,), 1.0, 40)
    st = T.AdamWState(p)
    g = _f16((100003,), 1e-3, 41)
    g[::1000] = 6.0e-8                             # subnormal gradients are gradients
    lp = p.clone()
    for _ in range(3):
        T.adamw_step(st, g, lr=1e-2, param_lp=lp)
    assert lp.dtype == F16 and torch.equal(lp, st.master.to(F16))
    assert not torch.equal(lp, p)


@pytest.mark.parametrize("bad", [float("inf"), float("nan"), -float("inf")])
def test_adamw_skips_on_a_non_finite_norm_bitwise(dev, bad):
    from haff import train_ops as T
    p = _f16((4096, 64), 1.0, 42)
    st = T.AdamWState(p)
    g = _f16((4096, 64), 1e-2, 43)
    lp = p.clone()
    T.adamw_step(st, g, lr=1e-3, param_lp=lp)      # non-zero moments first
    before = [t.clone() for t in (st.master, st.m, st.v, lp)]
    g2 = g.clone()
    g2[17, 3] = bad                                # one element: the norm of the f16 gradient is not finite
    norm = T.grad_norm([g2])
    assert not torch.isfinite(norm).item()
    clip = T.clip_coef_device(norm, 1.0)
    T.adamw_step(st, g2, lr=1e-3, param_lp=lp, gscale_dev=clip, skip_norm=norm)
    T.adamw_step(st, g2, lr=1e-3, param_lp=lp, skip_norm=norm)
    for a, b in zip((st.master, st.m, st.v, lp), before):
        assert torch.equal(a.view(torch.int16) if a.dtype == F16 else a.view(torch.int32),
                           b.view(torch.int16) if b.dtype == F16 else b.view(torch.int32))
    # a finite norm (values near 65504 included) takes the step, bit for bit as the plain dev-scale entry point
    g3 = g.clone()
    g3[0, 0] = 65504.0
    n3 = T.grad_norm([g3])
    assert torch.isfinite(n3).item()
    s_a, s_b = T.AdamWState(p), T.AdamWState(p)
    c3 = T.clip_coef_device(n3, 1.0)
    lp_a, lp_b = p.clone(), p.clone()
    T.adamw_step(s_a, g3, lr=1e-3, param_lp=lp_a, gscale_dev=c3, skip_norm=n3)
    T.adamw_step(s_b, g3, lr=1e-3, param_lp=lp_b, gscale_dev=c3)
    assert torch.equal(s_a.master, s_b.master) and torch.equal(lp_a, lp_b) and not torch.equal(lp_a, p)
