"""fp16 instances of the 16-bit kernels (f16 MFMA, fp32 accumulation) against torch on the same fp16 operands.

Exact layout check: small-integer operands (|v| <= 4) make every partial sum an integer below 2^24, so whatever the MFMA rounding,
the f32-output product must EQUAL the exact product and the f16-output product torch's round-to-nearest-even of it — at the shapes
the model multiplies (ViT-H, CLIP, Llama 7B / 13B at prefill and decode rows, reaching the 8-wave / 4-wave tiles, the weight-streaming
kernel and the split-K paths). A wrong fragment, swizzle or epilogue index cannot pass it, independently of arithmetic error.
Random operands: fp16 output is one rounding of an fp32 accumulator (half an ulp: 2^-11 |y|) plus accumulation order. Measured on
MI355X over the shapes below: max |err| / max |y| 2.6e-4 ... 4.2e-4; the bound is 1e-3 max |y| (2.4x the largest). Attention and norms:
fp32 torch on the same fp16 inputs."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

F16 = torch.float16

# (M, N, K) of the products the fp16 path runs
VIT = [(4096, 3840, 1280), (4096, 1280, 1280), (4096, 5120, 1280), (4096, 1280, 5120), (2 * 4096 + 40, 1280, 1280)]
CLIP = [(514, 3072, 1024), (514, 1024, 1024), (514, 4096, 1024), (514, 1024, 4096)]
LLAMA = {"7b": (4096, 11008), "13b": (5120, 13824)}
ROWS = [291, 1, 3, 8, 33, 64]


def _ints(shape, dev, seed):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return torch.randint(-4, 5, shape, generator=g, device=dev).to(F16)


def _exact_case(dev, M, N, K, seed, swiglu=False):
    from haff import ops
    x, w = _ints((M, K), dev, seed), _ints((N, K), dev, seed + 1)
    exact = (x.double() @ w.double().T)
    assert exact.abs().max().item() < 2 ** 24
    y32 = ops.linear(x, w, out_dtype=torch.float32)
    assert torch.equal(y32, exact.float()), (M, N, K)
    y16 = ops.linear(x, w)
    assert y16.dtype == F16 and torch.equal(y16, exact.float().to(F16)), (M, N, K)


@pytest.mark.parametrize("M,N,K", VIT + CLIP)
def test_f16_gemm_exact_layout_encoders(dev, M, N, K):
    _exact_case(dev, M, N, K, M + N + K)


@pytest.mark.parametrize("model", ["7b", "13b"])
@pytest.mark.parametrize("M", ROWS)
def test_f16_gemm_exact_layout_llama(dev, model, M):
    H, F = LLAMA[model]
    for N, K in ((3 * H, H), (H, H), (2 * F, H), (H, F)):   # q|k|v, o_proj, gate|up, down_proj
        _exact_case(dev, M, N, K, 7 * M + N)


def test_f16_gemm_exact_layout_forced_tiles(dev):
    from haff import ops
    x, w = _ints((1000, 1024), dev, 3), _ints((768, 1024), dev, 4)
    exact = (x.double() @ w.double().T).float()
    for cfg in (1, 2, 3):
        assert torch.equal(ops.linear(x, w, out_dtype=torch.float32, tile_cfg=cfg), exact), cfg
        assert torch.equal(ops.linear(x, w, tile_cfg=cfg), exact.to(F16)), cfg


def _rand(shape, dev, seed, scale=1.0):
    g = torch.Generator(device=dev)
    g.manual_seed(seed)
    return (torch.randn(shape, generator=g, device=dev) * scale).to(F16)


@pytest.mark.parametrize("M,N,K,act,swiglu,res", [
    (4096, 5120, 1280, 1, False, False),    # ViT-H lin1 + GELU
    (4096, 1280, 5120, 0, False, True),     # lin2 + residual
    (514, 3072, 1024, 2, False, False),     # CLIP fc1 + quick-GELU
    (291, 22016, 4096, 0, True, False),     # gate|up SwiGLU, prefill
    (3, 22016, 4096, 0, True, False),       # ... decode rows
    (64, 4096, 11008, 0, False, True),      # down_proj at 64 rows (split-K)
    (300, 4096, 11008, 0, False, True),     # prefill-sized down_proj (split-K tile path)
    (8, 12288, 4096, 0, False, False),      # q|k|v at decode rows
])
def test_f16_gemm_random_operands(dev, M, N, K, act, swiglu, res):
    from haff import ops
    x, w = _rand((M, K), dev, 1), _rand((N, K), dev, 2, K ** -0.5)
    bias = torch.randn((N,), device=dev) * 0.1
    n_out = N // 2 if swiglu else N
    if swiglu:   # rows interleaved in 16-row [gate | up] groups
        bias = None
    resid = _rand((M, n_out), dev, 3) if res else None
    y = ops.linear(x, w, bias=bias, act=act, resid=resid, swiglu=swiglu)
    acc = x.float() @ w.float().T
    if bias is not None:
        acc = acc + bias
    if swiglu:
        a = acc.view(M, N // 32, 2, 16)
        acc = (torch.nn.functional.silu(a[:, :, 0]) * a[:, :, 1]).reshape(M, n_out)
    elif act == 1:
        acc = torch.nn.functional.gelu(acc)
    elif act == 2:
        acc = acc * torch.sigmoid(1.702 * acc)
    if resid is not None:
        acc = acc + resid.float()
    err = (y.float() - acc).abs()
    scale = acc.abs().max().item()
    print(f"f16 gemm {M}x{N}x{K}: max rel err {(err / (acc.abs() + 1e-3 * scale)).max().item():.3e}, max|err|/scale {err.max().item() / scale:.3e}")
    assert torch.isfinite(y).all()
    assert err.max().item() <= 1e-3 * scale


def _attn_ref(q, k, v, scale, causal=False, q_pos0=0, bias=None):
    s = (q.float() @ k.float().transpose(-1, -2)) * scale
    if bias is not None:
        s = s + bias
    if causal:
        Nq, Nk = s.shape[-2:]
        i = torch.arange(Nq, device=s.device)[:, None] + q_pos0
        j = torch.arange(Nk, device=s.device)[None, :]
        s = s.masked_fill(j > i, float("-inf"))
    return torch.softmax(s, -1) @ v.float()


def _check_attn(out, ref, what, rel=4e-3):
    B, H, Nq, d = ref.shape
    ref = ref.permute(0, 2, 1, 3).reshape(B, Nq, H * d)
    err = (out.float() - ref).abs().max().item()
    scale = ref.abs().max().item()
    print(f"{what}: max|err| {err:.3e} of scale {scale:.3f}")
    assert out.dtype == F16 and err <= rel * scale, (what, err, scale)


@pytest.mark.parametrize("B,H,Nq,Nk,d,causal,q_pos0", [
    (2, 16, 257, 257, 64, False, 0),     # CLIP ViT-L
    (2, 4, 291, 291, 128, True, 0),      # Llama prefill
    (1, 4, 40, 300, 128, True, 260),     # a chunk appended behind a cache
])
def test_f16_flash_attention(dev, B, H, Nq, Nk, d, causal, q_pos0):
    from haff import ops
    q, k, v = _rand((B, H, Nq, d), dev, 11), _rand((B, H, Nk, d), dev, 12), _rand((B, H, Nk, d), dev, 13)
    out = ops.attention(q, k, v, d ** -0.5, causal=causal, q_pos0=q_pos0)
    _check_attn(out, _attn_ref(q, k, v, d ** -0.5, causal, q_pos0), f"flash {B}x{H}x{Nq}x{Nk}x{d}")


@pytest.mark.parametrize("S,B,H", [(14, 3, 4), (64, 1, 2)])
def test_f16_relpos_attention(dev, S, B, H):
    """SAM windowed (S = 14) and global (S = 64) attention of the fp16 path: haff_relpos_tables (dtype 3) + haff_attention_f16."""
    from haff import ops
    d, N = 80, S * S
    q, k, v = _rand((B, H, N, d), dev, 21), _rand((B, H, N, d), dev, 22), _rand((B, H, N, d), dev, 23)
    tab_h, tab_w = torch.randn((2 * S - 1, d), device=dev) * 0.1, torch.randn((2 * S - 1, d), device=dev) * 0.1
    relh, relw = ops.relpos_tables(q, tab_h, tab_w, S)
    qi = torch.arange(N, device=dev)
    qh, qw = qi // S, qi % S
    kk = torch.arange(S, device=dev)
    rh = torch.einsum("bhnd,nkd->bhnk", q.float(), tab_h[qh[:, None] - kk[None, :] + S - 1])
    rw = torch.einsum("bhnd,nkd->bhnk", q.float(), tab_w[qw[:, None] - kk[None, :] + S - 1])
    assert (relh.view(B, H, N, S) - rh).abs().max().item() <= 1e-4 * rh.abs().max().item() + 1e-5
    assert (relw.view(B, H, N, S) - rw).abs().max().item() <= 1e-4 * rw.abs().max().item() + 1e-5
    out = ops.attention(q, k, v, d ** -0.5, relh=relh, relw=relw, S=S)
    bias = (rh[..., :, None] + rw[..., None, :]).reshape(B, H, N, N)
    _check_attn(out, _attn_ref(q, k, v, d ** -0.5, bias=bias), f"relpos S={S}")


@pytest.mark.parametrize("B", [1, 3, 64, 160])   # B * H = 8, 24 (16-wave split), 512 (4-wave split), 1280 (one wave per head)
def test_f16_decode_attention(dev, B):
    """Llama decode rows: haff_attention_decode_rows_f16 on ragged caches, and the fused RoPE + cache append form
    (haff_decode_attention_rope_rows_f16) bit-identical to rope_cache_rows + decode rows (outputs and caches) in every wave layout."""
    from haff import ops
    H, d, Tmax = 8, 128, 320
    g = torch.Generator().manual_seed(B)
    nk = torch.randint(1, Tmax, (B,), generator=g).to(torch.int32).to(dev)
    kc, vc = _rand((B, Tmax, H * d), dev, 31), _rand((B, Tmax, H * d), dev, 32)
    q = _rand((B, 1, H * d), dev, 33)
    q4 = q.view(B, 1, H, d).permute(0, 2, 1, 3)
    k4 = kc.view(B, Tmax, H, d).permute(0, 2, 1, 3)
    v4 = vc.view(B, Tmax, H, d).permute(0, 2, 1, 3)
    out = ops.attention_decode_rows(q4, k4, v4, d ** -0.5, nk)
    for b in range(B):
        n = int(nk[b])
        ref = _attn_ref(q4[b:b + 1], k4[b:b + 1, :, :n], v4[b:b + 1, :, :n], d ** -0.5)
        _check_attn(out[b:b + 1], ref, f"decode rows b={b}")
    # fused RoPE + append vs the two kernels
    inv = 1.0 / (10000.0 ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
    ang = torch.arange(Tmax, dtype=torch.float32)[:, None] * inv[None, :]
    cs = torch.cat([torch.cos(ang), torch.sin(ang)], 1).contiguous().to(dev)
    qkv = _rand((B, 3 * H * d), dev, 34)
    k1, v1, k2, v2 = kc.clone(), vc.clone(), kc.clone(), vc.clone()
    fused = ops.decode_attention_rope(qkv, k1, v1, cs, H, d, d ** -0.5, nk)
    qkv2 = qkv.clone()
    ops.rope_cache_rows(qkv2, k2, v2, cs, B, 1, H, H, d, nk - 1)
    two = ops.attention_decode_rows(qkv2.view(B, 1, 3, H, d)[:, :, 0].permute(0, 2, 1, 3), k2.view(B, Tmax, H, d).permute(0, 2, 1, 3),
                                    v2.view(B, Tmax, H, d).permute(0, 2, 1, 3), d ** -0.5, nk)
    assert torch.equal(k1, k2) and torch.equal(v1, v2)
    assert torch.equal(fused, two)


@pytest.mark.parametrize("R,C", [(4096, 1280), (291, 4096), (7, 1024)])
def test_f16_norms(dev, R, C):
    from haff import ops
    x = _rand((R, C), dev, 41, 3.0)
    w, b = torch.randn((C,), device=dev), torch.randn((C,), device=dev)
    y = ops.layernorm(x, w, b, 1e-6)
    ref = torch.nn.functional.layer_norm(x.float(), (C,), w, b, 1e-6)
    assert y.dtype == F16 and (y.float() - ref).abs().max().item() <= 2e-3 * ref.abs().max().item()
    y = ops.rmsnorm(x, w, 1e-5)
    ref = x.float() * torch.rsqrt(x.float().pow(2).mean(-1, keepdim=True) + 1e-5) * w
    assert y.dtype == F16 and (y.float() - ref).abs().max().item() <= 2e-3 * ref.abs().max().item()
    st = ops.row_stats(x, 1e-6)
    xf = x.float()
    assert torch.allclose(st[:, 0], xf.mean(-1), atol=1e-4, rtol=1e-4)
    assert torch.allclose(st[:, 1], torch.rsqrt(xf.var(-1, unbiased=False) + 1e-6), rtol=1e-4)
    a = ops.add_bcast(x, x[:3].contiguous(), mod=3)
    assert torch.equal(a, (x.float() + x[:3].float().repeat(math.ceil(R / 3), 1)[:R]).to(F16))


def test_f16_fused_window_and_global_attention(dev):
    """haff_window_attention_f16 (28 windowed ViT-H blocks) and haff_global_attention_f16 (the 4 global ones): rel-pos inside the
    kernel from f16 tables, against fp32 torch on the same f16 inputs and f16-rounded tables."""
    from haff import ops
    d, H = 80, 2
    for S, nb in ((14, 3), (64, 1)):
        N = S * S
        qkv = _rand((nb, N, 3, H, d), dev, 50 + S)
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        tab_h, tab_w = torch.randn((2 * S - 1, d), device=dev) * 0.1, torch.randn((2 * S - 1, d), device=dev) * 0.1
        if S == 14:
            assert ops.window_attention_supported(q, S)
            out = ops.window_attention(q, k, v, d ** -0.5, tab_h, tab_w, S)
        else:
            assert ops.global_attention_supported(q, k, v, S)
            out = ops.global_attention(q, k, v, d ** -0.5, tab_h, tab_w, S)
        th, tw = tab_h.to(F16).float(), tab_w.to(F16).float()
        qi = torch.arange(N, device=dev)
        kk = torch.arange(S, device=dev)
        rh = torch.einsum("bhnd,nkd->bhnk", q.float(), th[(qi // S)[:, None] - kk[None, :] + S - 1])
        rw = torch.einsum("bhnd,nkd->bhnk", q.float(), tw[(qi % S)[:, None] - kk[None, :] + S - 1])
        bias = (rh[..., :, None] + rw[..., None, :]).reshape(nb, H, N, N)
        _check_attn(out, _attn_ref(q, k, v, d ** -0.5, bias=bias), f"fused rel-pos attention S={S}")


def test_f16_fused_products(dev):
    """The f16 instances of the fused products against the plain f16 product plus the separate kernel they replace."""
    from haff import ops
    # q|k|v + RoPE + cache append (prefill)
    B, T, H, d, K, Tmax = 4, 291, 4, 128, 1024, 320
    x, w = _rand((B * T, K), dev, 60), _rand((3 * H * d, K), dev, 61, K ** -0.5)
    inv = 1.0 / (10000.0 ** (torch.arange(0, d, 2, dtype=torch.float32) / d))
    ang = torch.arange(Tmax, dtype=torch.float32)[:, None] * inv[None, :]
    cs = torch.cat([torch.cos(ang), torch.sin(ang)], 1).contiguous().to(dev)
    kc1, vc1 = torch.zeros((B, Tmax, H * d), dtype=F16, device=dev), torch.zeros((B, Tmax, H * d), dtype=F16, device=dev)
    kc2, vc2 = kc1.clone(), vc1.clone()
    assert ops.qkv_rope_supported(B * T, H, d, K, F16, 1)
    q1 = ops.qkv_rope(x, ops.rope_permute_rows(w), kc1, vc1, cs, B, T, H, d, 7)
    qkv = ops.linear(x, w)
    ops.rope_cache(qkv, kc2, vc2, cs, B, T, H, H, d, 7)
    for a, b in ((q1, qkv[:, :H * d]), (kc1, kc2), (vc1, vc2)):
        err = (a.float() - b.float()).abs().max().item()
        assert err <= 2e-3 * b.float().abs().max().item(), err
    # folded LayerNorm (ln_stats / colsum) and producer row statistics
    M, C, N = 512, 1280, 3840
    h = _rand((M, C), dev, 62, 2.0)
    g, beta = torch.randn((C,), device=dev), torch.randn((C,), device=dev) * 0.1
    wq, bq = _rand((N, C), dev, 63, C ** -0.5), torch.randn((N,), device=dev) * 0.1
    wf, cs_, bf_ = ops.fold_norm(wq, g, beta, bq, F16)
    y1 = ops.linear(h, wf, bias=bf_, ln_stats=ops.row_stats(h, 1e-6), ln_colsum=cs_)
    y2 = ops.linear(ops.layernorm(h, g, beta, 1e-6), wq, bias=bq)
    assert (y1.float() - y2.float()).abs().max().item() <= 1e-2 * y2.float().abs().max().item()
    w2, b2 = _rand((C, C), dev, 64, C ** -0.5), torch.randn((C,), device=dev) * 0.1
    assert ops.linear_rowstats_supported(M, C, C, F16, 0)
    r1 = h.clone()
    out, st = ops.linear_rowstats(h, w2, b2, r1, 1e-6, out=r1)
    ref = ops.linear(h, w2, bias=b2, resid=h)
    assert (out.float() - ref.float()).abs().max().item() <= 2e-3 * ref.float().abs().max().item()
    assert torch.allclose(st, ops.row_stats(out, 1e-6), rtol=1e-4, atol=1e-4)   # the producer's statistics of the rows it wrote
    # RMSNorm carried between decode products (ssq partials) against rmsnorm + plain product
    Hd = 4096
    xr = _rand((3, Hd), dev, 65)
    n1 = torch.randn((Hd,), device=dev).abs() + 0.5
    wr = _rand((3 * Hd, Hd), dev, 66, Hd ** -0.5)
    wrf = (wr.float() * n1[None, :]).to(F16)
    ssq = torch.zeros((Hd // 16, 16), device=dev)
    ssq[0, :3] = xr.float().pow(2).sum(1)
    y1 = ops.linear_rms(xr, wrf, ssq_in=ssq[:1], eps=1e-5)
    y2 = ops.linear(ops.rmsnorm(xr, n1, 1e-5), wr)
    assert (y1.float() - y2.float()).abs().max().item() <= 1e-2 * y2.float().abs().max().item()
