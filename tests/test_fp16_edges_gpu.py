"""fp16 numeric edges of the f16 kernels, with operands built so that the exact result is known.

Every GEMM case runs through each dispatch branch the fp16 mode can take (BRANCHES below): the weight-streaming kernel with
MT = 1, 2 and 4 row tiles, its split-K form, the split-K tile path (gemm + skinny_reduce_kernel), the 128 x 128, 256 x 256 and
192 x 256 tiles, a specialised 256 x 256 epilogue instance, the producer of LayerNorm statistics (linear_rowstats) and the
q|k|v + RoPE product (qkv_rope, with an identity rotation so its outputs are the plain product).

- Subnormal operands: W (or A, or a mix of both) holds fp16 subnormals (< 2^-14). Every partial sum is a multiple of a power of
  two and bounded so that fp32 holds it exactly: the f32 output must EQUAL the exact product, the f16 output torch's IEEE
  conversion of it. An MFMA that flushed f16 subnormal inputs would give zeros.
- Rounding and range: exact integer results in (2048, 4096) (odd ones are ties in f16) and around +-65504 / 65520 / 69632. The
  f16 output must equal torch's round-to-nearest-even conversion, inf from 65520 on: round-toward-zero or saturation fails.
- Epilogue order: accumulators beyond fp16 range that a bias and / or residual brings back into range (exact), and GELU /
  SwiGLU of pre-activations beyond range whose output is in range (within one f16 rounding). Any path that rounds the
  accumulator to f16 before the epilogue gives inf.
- Subnormal softmax mass: one key per query at +D, every other key at 0, e^-D in [2^-24, 2^-14): the probabilities of the other
  keys are f16 subnormals when P is packed for the P.V MFMA, and v = 0 on the big key makes the output that mass alone.
"""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

F16 = torch.float16
SUB = 2.0 ** -14   # smallest normal fp16

# name -> (M, N, K, tile_cfg). Each shape reaches the branch of gemm_bf16_impl named.
BRANCHES = {
    "skinny_mt1_m1": (1, 1024, 1024, 0),
    "skinny_mt1": (16, 1024, 1024, 0),
    "skinny_mt2": (17, 1024, 1024, 0),
    "skinny_mt2_m32": (32, 1024, 1024, 0),
    "skinny_mt4": (48, 1024, 1024, 0),           # 33..64 rows, too few workgroups for the K split
    "skinny_mt4_splitk": (48, 4096, 4096, 0),    # launch_skinny_splitk + skinny_reduce_kernel
    "tile_splitk": (288, 1024, 4096, 0),         # 128 x 128 tile over K slices + skinny_reduce_kernel
    "tile128": (300, 520, 256, 1),
    "tile256": (512, 520, 256, 2),               # N % 256 != 0: the generic instance
    "tile256_spec": (512, 512, 256, 2),          # f16 output, whole N tiles: a specialised (GF_SPEC) instance
    "tile192": (400, 512, 256, 3),               # the HAFF_SPEC192 instances
}


def _dispatch(M, N, K, tile_cfg):
    """The branch gemm_bf16_impl takes for an f16 ops.linear() without maps or folded norms: a Python mirror of its rules
    (csrc/gemm_bf16.hip), so that a change of those thresholds shows up here instead of silently moving a case to another branch.
    linear() passes the 64 MiB workspace for 32 < M <= 1024 rows (haff_gemm_f16_ws) and none otherwise."""
    ws = 32 < M <= 1024 and not tile_cfg
    ws_bytes = 64 << 20
    tile_rows = M > 32 and ws and K % 64 == 0 and (N >= 8192 or K >= 8192)
    if M <= 64 and K % 128 == 0 and not tile_cfg and not (M > 32 and N >= 16384) and not tile_rows:
        if M > 32 and ws and ws_bytes >= 16 * M * N and N <= 8192:   # launch_skinny_splitk's admission
            tiles = (N + 15) // 16
            for nt in (4, 2):
                if any(K % (128 * ks) == 0 and 192 <= (tiles + nt - 1) // nt * ks <= 640 for ks in (4, 2)):
                    return "skinny_splitk"
        return "skinny_mt1" if M <= 16 else "skinny_mt2" if M <= 32 else "skinny_mt4"
    if not tile_cfg and ws and M > 32 and K % 64 == 0:                # split-K over the 128 x 128 tile
        t128, ksteps = -(-M // 128) * -(-N // 128), K // 64
        if t128 <= 256 and ksteps >= 32:
            for c in (16, 8, 4, 2):
                kc = -(-ksteps // c)
                n_sl = -(-ksteps // kc)
                if kc >= 4 and ksteps - (n_sl - 1) * kc >= 2 and t128 * n_sl <= 512 and 4 * n_sl * M * N <= ws_bytes:
                    return "tile_splitk"
    return {1: "tile128", 2: "tile256", 3: "tile192"}.get(tile_cfg, "auto")


# the branch each BRANCHES entry must reach
DISPATCH = {"skinny_mt1_m1": "skinny_mt1", "skinny_mt1": "skinny_mt1", "skinny_mt2": "skinny_mt2", "skinny_mt2_m32": "skinny_mt2",
            "skinny_mt4": "skinny_mt4", "skinny_mt4_splitk": "skinny_splitk", "tile_splitk": "tile_splitk", "tile128": "tile128",
            "tile256": "tile256", "tile256_spec": "tile256", "tile192": "tile192"}


def _reaches(branch):
    M, N, K, cfg = BRANCHES[branch]
    assert _dispatch(M, N, K, cfg) == DISPATCH[branch], (branch, _dispatch(M, N, K, cfg))
    return M, N, K, cfg


def _ops():
    import haff  # noqa: F401
    from haff import ops
    return ops


def _ints(shape, seed, lo=-4, hi=4, nonzero=False):
    g = torch.Generator().manual_seed(seed)
    v = torch.randint(lo, hi + 1, shape, generator=g)
    if nonzero:
        v[v == 0] = 1
    return v.double()


def _check_exact_bound(a, w, gran):
    """every partial sum of a @ w.T is a multiple of gran and bounded by |a| @ |w|.T: fp32 holds it exactly below 2^24 gran"""
    assert (a.abs() @ w.abs().T).max().item() < 2.0 ** 24 * gran


def _operands(kind, M, N, K, seed):
    """(a, w) float64 on the CPU, exactly representable in fp16."""
    if kind == "sub_w":        # W = +-(1..15) 2^-20: every element an fp16 subnormal
        a, w = _ints((M, K), seed), _ints((N, K), seed + 1, -15, 15, nonzero=True) * 2.0 ** -20
        gran = 2.0 ** -20
    elif kind == "sub_a":      # the mirror case
        a, w = _ints((M, K), seed, -15, 15, nonzero=True) * 2.0 ** -20, _ints((N, K), seed + 1)
        gran = 2.0 ** -20
    elif kind == "mixed":      # both operands mix subnormal (+-(1..7) 2^-17) and normal (+-(1..3) 2^-14) elements
        def mix(shape, s):
            sub = _ints(shape, s + 7, 0, 1) > 0
            return torch.where(sub, _ints(shape, s, -7, 7, nonzero=True) * 2.0 ** -17, _ints(shape, s + 3, -3, 3, nonzero=True) * 2.0 ** -14)
        a, w = mix((M, K), seed), mix((N, K), seed + 1)
        gran = 2.0 ** -34
    elif kind == "round":      # integer results needing rounding in f16: ties in (2048, 4096) and the overflow band, both signs
        a, w = _ints((M, K), seed), _ints((N, K), seed + 1)
        a[:, 0] = 2048.0
        base = torch.tensor([1.5, -1.5, 32.0, -32.0, 34.0, -34.0, 1.0, -1.0], dtype=torch.float64)
        w[:, 0] = base[torch.arange(N) % 8]
        gran = 1.0
    else:
        raise ValueError(kind)
    assert torch.equal(a.to(F16).double(), a) and torch.equal(w.to(F16).double(), w)
    _check_exact_bound(a, w, gran)
    return a, w


def _check_operands_are_subnormal(kind, a, w):
    for t, name in ((a, "a"), (w, "w")):
        n_sub = ((t != 0) & (t.abs() < SUB)).sum().item()
        if kind == "sub_w" and name == "w" or kind == "sub_a" and name == "a":
            assert n_sub == t.numel()
        if kind == "mixed":
            assert 0.3 * t.numel() < n_sub < 0.7 * t.numel()


def _ulp16(x):
    """one fp16 ulp at |x| (the subnormal spacing 2^-24 below 2^-14)"""
    e = torch.floor(torch.log2(x.abs().clamp_min(SUB)))
    return torch.pow(2.0, e - 10)


@pytest.mark.parametrize("kind", ["sub_w", "sub_a", "mixed", "round"])
@pytest.mark.parametrize("branch", list(BRANCHES))
def test_f16_gemm_exact_edges(dev, branch, kind):
    """Subnormal operands (W, A, both) and results that need IEEE rounding (ties, +-65504 / 65520 / 69632) on every GEMM branch:
    haff_gemm_f16 / _f16_cfg / _f16_ws -> gemm_skinny_kernel<MT=1,2,4>, skinny_reduce_kernel, gemm_bf16_kernel 128 / 256 / 192
    tiles, generic and specialised epilogues. f32 output == exact; f16 output == torch's conversion of exact."""
    ops = _ops()
    M, N, K, cfg = _reaches(branch)
    a, w = _operands(kind, M, N, K, M + N + K)
    _check_operands_are_subnormal(kind, a, w)
    exact = a @ w.T
    x, wt = a.to(F16).to(dev), w.to(F16).to(dev)
    want16 = exact.float().to(F16)
    if kind == "round":
        assert torch.isinf(want16).any() and (want16.abs() == 65504).any()
        ties = (exact.abs() > 2048) & (exact.abs() < 4096) & (exact % 2 == 1)
        assert ties.sum().item() > 0.05 * exact.numel()
    else:
        assert (exact != 0).float().mean().item() > 0.9    # a flushing MFMA gives zeros
    if branch != "tile256_spec":   # the specialised instances have no f32-output form
        y32 = ops.linear(x, wt, out_dtype=torch.float32, tile_cfg=cfg)
        assert torch.equal(y32.cpu(), exact.float()), (branch, kind, (y32.cpu().double() - exact).abs().max().item())
    y16 = ops.linear(x, wt, tile_cfg=cfg)
    assert y16.dtype == F16
    bad = (y16.cpu() != want16).sum().item()
    assert torch.equal(y16.cpu(), want16), (branch, kind, f"{bad} of {want16.numel()} differ")


@pytest.mark.parametrize("kind", ["sub_w", "mixed", "round"])
def test_f16_rowstats_and_qkv_rope_exact_edges(dev, kind):
    """The same exact operands through the fused producers: linear_rowstats (haff_gemm_f16_rowstats, bias + residual, and the
    statistics of the rows it wrote) and qkv_rope (haff_gemm_f16_qkv_rope with cos = 1, sin = 0: q and the cache rows are the plain
    product)."""
    ops = _ops()
    M, N, K = 512, 512, 256
    a, w = _operands(kind, M, N, K, 5)
    exact = a @ w.T
    bias = _ints((N,), 9).float() * (2.0 ** -20 if kind != "round" else 1.0)
    resid = _ints((M, N), 10).to(F16) * (2.0 ** -20 if kind != "round" else 1.0)
    want = (exact + bias.double() + resid.double()).float().to(F16)
    if kind == "round":
        assert torch.isinf(want).any()
    x, wt = a.to(F16).to(dev), w.to(F16).to(dev)
    out, st = ops.linear_rowstats(x, wt, bias.to(dev), resid.to(dev), 1e-6)
    assert torch.equal(out.cpu(), want)
    if kind != "round":
        assert torch.allclose(st, ops.row_stats(out, 1e-6), rtol=1e-4, atol=1e-4)

    B, T, H, d = 2, 256, 2, 128
    Kq = 256
    a, w = _operands(kind, B * T, 3 * H * d, Kq, 6)
    exact = (a @ w.T).float().to(F16)
    Tmax, pos0 = 300, 5
    cs = torch.cat([torch.ones((Tmax, d // 2)), torch.zeros((Tmax, d // 2))], 1).contiguous().to(dev)
    kc = torch.zeros((B, Tmax, H * d), dtype=F16, device=dev)
    vc = torch.zeros_like(kc)
    x, wt = a.to(F16).to(dev), w.to(F16).to(dev)
    assert ops.qkv_rope_supported(B * T, H, d, Kq, F16, 1)
    q = ops.qkv_rope(x, ops.rope_permute_rows(wt), kc, vc, cs, B, T, H, d, pos0)
    Hd = H * d
    assert torch.equal(q.cpu(), exact[:, :Hd])
    assert torch.equal(kc[:, pos0:pos0 + T].cpu(), exact[:, Hd:2 * Hd].view(B, T, Hd))
    assert torch.equal(vc[:, pos0:pos0 + T].cpu(), exact[:, 2 * Hd:].view(B, T, Hd))


# branches with an epilogue: name -> (M, N, K, tile_cfg)
EPI_BRANCHES = {k: BRANCHES[k] for k in ("skinny_mt1", "skinny_mt2", "skinny_mt4", "skinny_mt4_splitk", "tile_splitk", "tile128",
                                         "tile256", "tile256_spec", "tile192")}


def _big_acc_operands(M, N, K, seed, w0):
    """integer a, w with a[:, 0] = 2048 and w[:, 0] = w0 (per row): accumulators 2048 * w0 +- a few hundred"""
    a, w = _ints((M, K), seed), _ints((N, K), seed + 1)
    a[:, 0] = 2048.0
    w[:, 0] = w0
    _check_exact_bound(a, w, 1.0)
    return a, w


@pytest.mark.parametrize("epi", ["bias", "resid", "bias_resid"])
@pytest.mark.parametrize("branch", list(EPI_BRANCHES))
def test_f16_epilogue_in_fp32_exact(dev, branch, epi):
    """Accumulators of +-81920 (beyond 65504) brought back into range by an fp32 bias and / or an f16 residual: bias -> +resid in
    fp32, ONE rounding. Every value is an integer below 2^24, so the f16 output must EQUAL torch's conversion of the exact sum
    (gemm epilogues, skinny_reduce_kernel of both split-K forms, the 192-row and specialised instances)."""
    ops = _ops()
    M, N, K, cfg = _reaches(branch)
    sign = torch.where(torch.arange(N) % 2 == 0, 1.0, -1.0).double()
    a, w = _big_acc_operands(M, N, K, 3 * M + N, 40.0 * sign)
    acc = a @ w.T
    assert acc.abs().min().item() > 65520
    bias = resid = None
    want = acc.clone()
    if epi in ("bias", "bias_resid"):
        b = -sign * (24576.0 if epi == "bias_resid" else 40000.0)
        bias = b.float().to(dev)
        want = want + b
    if epi in ("resid", "bias_resid"):
        r = -sign[None, :].expand(M, N) * (24576.0 if epi == "bias_resid" else 32768.0)
        r = (r + _ints((M, N), 77)).to(F16)
        resid = r.to(dev)
        want = want + r.double()
    assert want.abs().max().item() < 65504
    want16 = want.float().to(F16)
    y = ops.linear(a.to(F16).to(dev), w.to(F16).to(dev), bias=bias, resid=resid, tile_cfg=cfg)
    assert torch.isfinite(y).all(), (branch, epi, (~torch.isfinite(y)).sum().item())
    assert torch.equal(y.cpu(), want16), (branch, epi)


@pytest.mark.parametrize("branch", ["skinny_mt1", "skinny_mt4_splitk", "tile_splitk", "tile128", "tile256", "tile256_spec", "tile192"])
def test_f16_gelu_of_out_of_range_accumulator(dev, branch):
    """GELU of pre-activations 2048 * 40 +- ... (beyond fp16 range) plus a residual of -32768 lands in range: act and residual in
    fp32, one rounding (gemm_act<GELU>, apply_act in skinny_reduce_kernel). Within one f16 ulp of the fp64 reference."""
    ops = _ops()
    M, N, K, cfg = _reaches(branch)
    a, w = _big_acc_operands(M, N, K, 5 * M + N, 40.0)
    acc = a @ w.T
    r = (torch.full((M, N), -32768.0, dtype=torch.float64) + _ints((M, N), 78)).to(F16).double()
    ref = torch.nn.functional.gelu(acc) + r
    y = ops.linear(a.to(F16).to(dev), w.to(F16).to(dev), act=1, resid=r.to(F16).to(dev), tile_cfg=cfg)
    assert torch.isfinite(y).all()
    err = (y.cpu().double() - ref).abs()
    assert (err <= _ulp16(ref)).all(), (branch, err.max().item())


@pytest.mark.parametrize("branch", ["skinny_mt1", "skinny_mt2", "tile_splitk", "tile128", "tile256", "tile192"])
def test_f16_swiglu_of_out_of_range_gate(dev, branch):
    """SwiGLU with gates of +-81920 (beyond fp16 range) and up rows of |u| < 0.8: silu(gate) * up in fp32, one rounding, output in
    range (gemm epilogue, skinny reduce of the split-K tile path). Within one f16 ulp of the fp64 reference."""
    ops = _ops()
    M, N, K, cfg = _reaches(branch)
    N = max(N // 32 * 32, 32)
    a = _ints((M, K), 11 + M)
    w = _ints((N, K), 12 + N)
    a[:, 0] = 2048.0
    row = torch.arange(N)
    gate = (row // 16) % 2 == 0   # rows interleaved [gate x16 | up x16]
    w[gate, 0] = torch.where((row[gate] // 32) % 2 == 0, 40.0, -40.0).double()
    w[~gate, 0] = 0.0
    m = (a @ w[~gate].T).abs().max().item()   # up rows scaled by 2^-sh: |silu(gate) * up| stays below 65504 / 1.1
    sh = math.ceil(math.log2(m * 2048 * 40 * 1.1 / 65504))
    w[~gate] = w[~gate] * 2.0 ** -sh
    _check_exact_bound(a, w[gate], 1.0)
    _check_exact_bound(a, w[~gate], 2.0 ** -sh)
    acc = (a @ w.T).view(M, N // 32, 2, 16)
    g, u = acc[:, :, 0], acc[:, :, 1]
    assert g.abs().min().item() > 65520
    ref = (torch.nn.functional.silu(g) * u).reshape(M, N // 2)
    assert ref.abs().max().item() < 65504 and (ref.abs() > 2048).float().mean().item() > 0.05
    y = ops.linear(a.to(F16).to(dev), w.to(F16).to(dev), swiglu=True, tile_cfg=cfg)
    assert torch.isfinite(y).all()
    err = (y.cpu().double() - ref).abs()
    assert (err <= _ulp16(ref)).all(), (branch, err.max().item())


# --- subnormal probability mass in attention --------------------------------------------------------------------------------

def _mass_qkv(B, H, Nk, d, Nq, big, delta, seed):
    """q = e_0, k = 0 except key `big` (score delta after scaling), v in [0.5, 1.5] except v[big] = 0: out = sum_j!=big p_j v_j,
    every such p_j = e^-delta / l an fp16 subnormal."""
    scale = d ** -0.5
    q = torch.zeros((B, H, Nq, d), dtype=torch.float64)
    q[..., 0] = 1.0
    k = torch.zeros((B, H, Nk, d), dtype=torch.float64)
    k[:, :, big, 0] = delta / scale
    g = torch.Generator().manual_seed(seed)
    v = torch.rand((B, H, Nk, d), generator=g, dtype=torch.float64) + 0.5
    v[:, :, big] = 0.0
    return q.to(F16), k.to(F16), v.to(F16), scale


def _mass_ref(q, k, v, scale, dev):
    s = (q.to(dev).double() @ k.to(dev).double().transpose(-1, -2)) * scale
    p = torch.softmax(s, -1)
    return p @ v.to(dev).double(), s


def _check_mass(out, ref, s, what, frac):
    """out [B, Nq, H*d] against ref [B, H, Nq, d]; frac: measured max|err| / the subnormal mass (output scale)"""
    B, H, Nq, d = ref.shape
    smax = s.max(-1, keepdim=True).values
    e = torch.exp(s - smax)
    small = (e < SUB) & (e > 0)
    assert ((e[small] >= 2.0 ** -24) & (e[small] < SUB)).all()
    mass = ((e * small).sum(-1) / e.sum(-1)).min().item()
    ref = ref.permute(0, 2, 1, 3).reshape(B, Nq, H * d)
    err = (out.double() - ref).abs().max().item()
    print(f"{what}: subnormal mass {mass:.4f}, max|err| {err:.3e} = {err / mass:.3e} of the mass")
    assert torch.isfinite(out).all()
    assert err <= frac * mass, (what, err, mass)


# measured on MI355X, max|err| / mass: flash 3.0e-3, window 3.4e-3, global 3.3e-3 (P packed to f16 for the P.V MFMA: relative
# rounding of 2^-11 plus subnormal spacing), decode rows and fused decode + RoPE 4.9e-4 (P in fp32). Bounds 2.5x those, far under
# the whole mass (what a flushed P loses).
MASS_MFMA, MASS_DECODE = 8.5e-3, 1.25e-3


def test_f16_flash_attention_subnormal_mass(dev):
    """haff_attention_f16 (flash, d = 64, 4096 keys): e^-11 = 1.7e-5 per non-max key, 6.4 % of the mass in subnormal P."""
    ops = _ops()
    B, H, N, d = 1, 2, 4096, 64
    q, k, v, scale = _mass_qkv(B, H, N, d, 256, 1234, 11.0, 1)
    out = ops.attention(q.to(dev), k.to(dev), v.to(dev), scale)
    ref, s = _mass_ref(q, k, v, scale, dev)
    _check_mass(out, ref, s, "flash f16", MASS_MFMA)


def test_f16_decode_attention_subnormal_mass(dev):
    """haff_attention_decode_rows_f16 and haff_decode_attention_rope_rows_f16 (cos = 1, sin = 0: the rotation is the identity) on
    ragged caches of up to 4000 keys."""
    ops = _ops()
    B, H, d, Tmax = 3, 8, 128, 4096
    nk = torch.tensor([4000, 3000, 2500], dtype=torch.int32)
    q, k, v, scale = _mass_qkv(B, H, Tmax, d, 1, 1000, 11.0, 2)
    kc = k.permute(0, 2, 1, 3).reshape(B, Tmax, H * d).contiguous().to(dev)
    vc = v.permute(0, 2, 1, 3).reshape(B, Tmax, H * d).contiguous().to(dev)
    k4 = kc.view(B, Tmax, H, d).permute(0, 2, 1, 3)
    v4 = vc.view(B, Tmax, H, d).permute(0, 2, 1, 3)
    out = ops.attention_decode_rows(q.to(dev), k4, v4, scale, nk.to(dev))
    for b in range(B):
        n = int(nk[b])
        ref, s = _mass_ref(q[b:b + 1], k[b:b + 1, :, :n], v[b:b + 1, :, :n], scale, dev)
        _check_mass(out[b:b + 1], ref, s, f"decode rows f16 b={b}", MASS_DECODE)
    # fused RoPE + cache append: the new key (row nk - 1) is 0 with v in [0.5, 1.5]
    cs = torch.cat([torch.ones((Tmax, d // 2)), torch.zeros((Tmax, d // 2))], 1).contiguous().to(dev)
    g = torch.Generator().manual_seed(3)
    qkv = torch.zeros((B, 3, H, d), dtype=torch.float64)
    qkv[:, 0, :, 0] = 1.0
    qkv[:, 2] = torch.rand((B, H, d), generator=g, dtype=torch.float64) + 0.5
    qkv = qkv.reshape(B, 3 * H * d).to(F16).to(dev)
    out = ops.decode_attention_rope(qkv, kc, vc, cs, H, d, scale, nk.to(dev))
    for b in range(B):
        n = int(nk[b])
        assert torch.equal(kc[b, n - 1], qkv[b, H * d:2 * H * d]) and torch.equal(vc[b, n - 1], qkv[b, 2 * H * d:])
        kk = kc[b:b + 1, :n].view(1, n, H, d).permute(0, 2, 1, 3).cpu()
        vv = vc[b:b + 1, :n].view(1, n, H, d).permute(0, 2, 1, 3).cpu()
        ref, s = _mass_ref(q[b:b + 1], kk, vv, scale, dev)
        _check_mass(out[b:b + 1], ref, s, f"decode+rope f16 b={b}", MASS_DECODE)


def test_f16_window_attention_subnormal_mass(dev):
    """haff_window_attention_f16 (14 x 14 windows, d = 80, rel-pos tables zero): e^-9.75 = 5.8e-5 per non-max key. 195 other
    keys cap the subnormal mass of a window at 195 * 2^-14 = 1.2 %; here it is 1.1 %."""
    ops = _ops()
    S, d, H, nw = 14, 80, 2, 8
    N = S * S
    q, k, v, scale = _mass_qkv(nw, H, N, d, N, 100, 9.75, 4)
    qkv = torch.stack([q, k, v], 2).to(dev)   # [nw, H, 3, N, d]
    qkv = qkv.permute(0, 3, 2, 1, 4).contiguous()   # [nw, N, 3, H, d]: the layout of the q|k|v product
    qd, kd, vd = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    zeros = torch.zeros((2 * S - 1, d), device=dev)
    out = ops.window_attention(qd, kd, vd, scale, zeros, zeros, S)
    ref, s = _mass_ref(q, k, v, scale, dev)
    _check_mass(out, ref, s, "window f16", MASS_MFMA)


def test_f16_global_attention_subnormal_mass(dev):
    """haff_global_attention_f16 (64 x 64 tokens, d = 80, rel-pos tables zero) as the product runs it, 16 heads x 2 frames:
    e^-11 per non-max key, 6.4 % of the mass."""
    ops = _ops()
    S, d, H, B = 64, 80, 16, 2
    N = S * S
    q, k, v, scale = _mass_qkv(B, H, N, d, N, 2100, 11.0, 5)
    qkv = torch.stack([q, k, v], 2).to(dev).permute(0, 3, 2, 1, 4).contiguous()
    qd, kd, vd = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    assert ops.global_attention_supported(qd, kd, vd, S)
    zeros = torch.zeros((2 * S - 1, d), device=dev)
    out = ops.global_attention(qd, kd, vd, scale, zeros, zeros, S)
    for b in range(B):
        for h0 in range(0, H, 4):
            hs = slice(h0, h0 + 4)
            ref, s = _mass_ref(q[b:b + 1, hs], k[b:b + 1, hs], v[b:b + 1, hs], scale, dev)
            _check_mass(out[b:b + 1].view(1, N, H, d)[:, :, hs].reshape(1, N, 4 * d), ref, s, f"global f16 frame {b} heads {h0}+",
                        MASS_MFMA)
