"""The inference attention kernels on inputs whose right answer is one row of V, or the mean of two (tests/attn_edge_ref.py, checked on
its own by tests/test_attn_edge_ref_cpu.py): the generic flash kernel by dispatch branch of attention_bf16_impl, the ViT-H global
ping-pong kernel with fp32 and with fused tables, the three decode layouts with and without fused RoPE, the window kernel past one
trip of its persistent loop and on padded grids, the two fp32 kernels. Every row of every case is compared (padded window positions,
which no caller reads, excepted). One-hot cases of the generic, decode and fp32 kernels are compared with ==; everything else is held
per element to u * |v| + one output ulp (attn_edge_ref.bound), a bound that comes from the formats and not from the kernels. Outputs go
through out= into a NaN-filled allocation with 64 guard columns and a guard row on either side, and the guards must keep their bits.
Operands come in the layouts the product uses: a token-major fused [B, N, 3, H, d] where Nq == Nk, a separate q with fused k | v
otherwise. Every case is a geometry its entry point admits, no operand leaves its documented contract, nothing is meant to fault."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_edge_ref as A   # noqa: E402

pytestmark = pytest.mark.gpu

UNSUPPORTED = -2
BF16, F16, F32, F64 = A.BF16, A.F16, A.F32, A.F64
_id = lambda v: A.IDS.get(v, None)   # noqa: E731
WORST = {}


def _ops():
    import haff  # noqa: F401
    from haff import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for name in sorted(WORST):
        print(f"WORST {name}: {WORST[name]:.3g} of the bound")


# ------------------------------------------------------------------------------------------------------------------ layouts
def _heads(buf, i):
    """[B, N, parts, H, d] -> the [B, H, N, d] view of part i"""
    return buf[:, :, i].permute(0, 2, 1, 3)


def _pack(parts, dev):
    """[B, H, N, d] tensors of one N -> one token-major fused allocation [B, N, len(parts), H, d] on the device and their views"""
    buf = torch.stack([p.permute(0, 2, 1, 3) for p in parts], 2).contiguous().to(dev)
    return [_heads(buf, i) for i in range(len(parts))]


def _operands(c, dev, split_kv=False):
    """q | k | v fused where Nq == Nk, q apart from a fused k | v otherwise; split_kv: k and v are two contiguous token-major
    tensors [B, Nk, H, d] of their own (same strides), v at the LOWER address, both carved from one allocation so that the order
    does not hang on the caching allocator"""
    if split_kv:
        buf = torch.stack([c.v.permute(0, 2, 1, 3), c.k.permute(0, 2, 1, 3)], 0).contiguous().to(dev)
        k, v = buf[1].permute(0, 2, 1, 3), buf[0].permute(0, 2, 1, 3)
        assert v.data_ptr() < k.data_ptr() and k.stride() == v.stride()
        return _pack([c.q], dev)[0], k, v
    if c.q.shape[2] == c.k.shape[2]:
        return _pack([c.q, c.k, c.v], dev)
    return [_pack([c.q], dev)[0]] + _pack([c.k, c.v], dev)


def _pp_admits(q, k, v, rel):
    """attn_global_pp_ok(p, false) of attention.hip restated on what the host can see, with the expression
    ops.global_attention_supported uses for the k | v layout: d 80, S 64, whole 256-query and 64-key tiles, at least two key tiles,
    equal k and v strides, v not below k, a span below 2^31 bytes, q / k / v / relh / relw 16-byte aligned. No test can see which
    kernel a launch took; this pins the branch by its admission rule."""
    if not rel or rel["S"] != 64 or q.shape[3] != 80 or q.shape[2] % 256 or k.shape[2] % 64 or k.shape[2] < 128:
        return False
    layout = (k.stride() == v.stride() and v.data_ptr() >= k.data_ptr()
              and (v.data_ptr() - k.data_ptr()) + k.shape[2] * k.stride(2) * 2 < (1 << 31))
    return layout and all(t.data_ptr() % 16 == 0 for t in (q, k, v, rel["relh"], rel["relw"]))


class Out:
    """the out= argument [B, Nq, H*d] as a view of a NaN-filled [B, Nq + 2, H*d + 64] allocation"""

    def __init__(self, B, Nq, H, d, dtype, dev):
        self.shape = (B, Nq, H, d)
        self.big = torch.full((B, Nq + 2, H * d + 64), A.NAN, dtype=dtype, device=dev)
        self.view = self.big[:, 1:Nq + 1, :H * d]

    def get(self):
        """-> [B, H, Nq, d] on the CPU, once the guard rows and columns are seen to hold their bits"""
        B, Nq, H, d = self.shape
        big = self.big.cpu()
        ints = big.view(torch.int32 if big.dtype == F32 else torch.int16)
        guard = torch.ones(big.shape, dtype=torch.bool)
        guard[:, 1:Nq + 1, :H * d] = False
        want = torch.full((1,), A.NAN, dtype=big.dtype).view(ints.dtype)
        assert bool((ints[guard] == want).all()), "a guard row or column was written"
        return big[:, 1:Nq + 1, :H * d].reshape(B, Nq, H, d).permute(0, 2, 1, 3)


def _rel(c, dev):
    if c.relh is None:
        return {}
    B, H, Nq, S = c.relh.shape
    return dict(relh=c.relh.reshape(B * H, Nq, S).contiguous().to(dev), relw=c.relw.reshape(B * H, Nq, S).contiguous().to(dev), S=S)


def _attention(c, dev, split_kv=False, twice=False, pingpong=False):
    """pingpong: whether the launch has to be one attn_global_pp_ok admits (asserted either way)"""
    ops = _ops()
    B, H, Nq, d = c.q.shape
    q, k, v = _operands(c, dev, split_kv)
    rel = _rel(c, dev)
    assert _pp_admits(q, k, v, rel) == pingpong, "the operands do not reach the branch this case is listed for"
    outs = []
    for _ in range(2 if twice else 1):
        o = Out(B, Nq, H, d, c.q.dtype, dev)
        ops.attention(q, k, v, c.scale, causal=c.causal, q_pos0=c.q_pos0, out=o.view, **rel)
        outs.append(o.get())
    if twice:
        assert torch.equal(outs[0], outs[1]), "a second launch gave other bits"
    return outs[0]


# ----------------------------------------------------------------------------------------------------------------- compare
def _where(bad, c):
    at = bad.nonzero()[:8].tolist()
    return [(tuple(i), int(c.choice[tuple(i)])) for i in at]


def _exact(got, c, what):
    """one-hot: out == the chosen V row, bit for bit"""
    want = c.v_choice()
    bad = (got != want).any(-1)
    print(f"{what}: {int(bad.sum())} of {bad.numel()} rows differ from the chosen V row")
    assert not bool(bad.any()), f"{what}: out is not the chosen V row at (b, h, query) -> choice {_where(bad, c)}"


def _bounded(got, c, u, name, what):
    ref = c.v_choice().double() if c.onehot else c.ref()
    r = (got.double() - ref).abs() / A.bound(ref, c.vmax, c.q.dtype, u)
    r = torch.where(torch.isnan(r), torch.full_like(r, A.INF), r)
    bad = r > 1.0
    if c.is_pad is not None:
        bad &= ~c.is_pad[:, None, :, None]
        r = r.permute(0, 2, 1, 3)[~c.is_pad]
    worst = float(r.max())
    WORST[name] = max(WORST.get(name, 0.0), worst)
    print(f"{name} {what}: {worst:.3g} of the bound")
    assert worst <= 1.0, f"{name} {what}: |err| / bound = {worst:.3g} at (b, h, query) -> choice {_where(bad.any(-1), c)}"


def _generic(c, dev, what, **kw):
    got = _attention(c, dev, **kw)
    if c.onehot:
        _exact(got, c, what)
    else:
        _bounded(got, c, A.U16[c.q.dtype], "generic", what)


# ---------------------------------------------------------------------------------------------------------- generic kernel
@pytest.mark.parametrize("dtype", A.HALF, ids=_id)
@pytest.mark.parametrize("d", (64, 72, 80, 104))
def test_generic_no_bias(dev, d, dtype):
    """attn_fwd_kernel<dp, 0, causal> at dp 64 (d 64), 96 (d 72: d % 16 != 0; d 80) and 128 (d 104): one key, a key tile one short
    and one over, a second query block of one row, Nq > Nk; at d 64 the causal instance with 0 < q_pos0 < Nk - Nq and q_pos0 = Nk - Nq
    and the grid decoded for B * H = 3 and 8 with two query blocks. One-hot rows ==, pairs and late jumps within the bound."""
    for t in A.GENERIC_PLAIN:
        if t[0] != d:
            continue
        _, B, H, Nq, Nk, causal, p0 = t
        what = f"{A.case_id(t)} {A.IDS[dtype]}"
        _generic(A.select_by_qk(B, H, Nq, Nk, d, Nq + Nk, dtype, bool(causal), p0), dev, "qk " + what)
        _generic(A.pair_inputs(B, H, Nq, Nk, d, Nq + Nk + 1, dtype, bool(causal), p0, first=64), dev, "pair " + what)
        if Nk > 81:
            _generic(A.pair_inputs(B, H, Nq, Nk, d, Nq + Nk + 2, dtype, bool(causal), p0, late_jump=True, first=64), dev, "late " + what)


@pytest.mark.parametrize("dtype", A.HALF, ids=_id)
@pytest.mark.parametrize("cases", (A.GENERIC_BIAS3, A.GENERIC_BIAS1, A.GENERIC_BIAS2), ids=("bias3", "bias1", "bias2"))
def test_generic_rel_pos(dev, cases, dtype):
    """fp32 relh / relw select the key. BIAS 3: S <= 16 and Nk = S * S (16-wide virtual key rows). BIAS 1: S = 3 (Nk 6), 14 with 13
    rows, 20, 32 (the LDS table). BIAS 2 off the ping-pong path: d 64, d 128 (bf16; f16 refuses rel-pos at d > 96, asserted as the
    return code), d 80 at Nq = 128 (FULL + LSUM) and Nq = 100 (LSUM, not FULL)."""
    ops = _ops()
    for t in cases:
        d, B, H, Nq, Nk, S = t
        c = A.select_by_bias(B, H, Nq, Nk, d, S, Nq + S, dtype)
        if dtype == F16 and d > 96:
            from haff.lib import load_library
            q, k, v = _operands(c, dev)
            o = Out(B, Nq, H, d, dtype, dev)
            qkvo, _ = ops._qkvo(q, k, v, o.view)
            rel = _rel(c, dev)
            rc = load_library().haff_attention_f16(*qkvo, B, H, Nq, Nk, d, float(c.scale), 0, 0, rel["relh"].data_ptr(), rel["relw"].data_ptr(), S,
                                                   torch.cuda.current_stream().cuda_stream)
            assert rc == UNSUPPORTED, rc
            torch.cuda.synchronize()
            assert bool(torch.isnan(o.big).all()), "a refused call wrote its output"
            continue
        _generic(c, dev, f"bias {A.case_id(t)} {A.IDS[dtype]}")


@pytest.mark.parametrize("dtype", A.HALF, ids=_id)
def test_generic_bias2_separate_k_and_v(dev, dtype):
    """d 80, S 64, Nq % 256 == 0, Nk = 128 with k and v as two tensors of equal strides, v at the lower address: attn_global_pp_ok
    asks for v >= k (not for one allocation), so it is false (asserted in _attention on the pointers) and the generic FULL + LSUM
    instance runs"""
    d, B, H, Nq, Nk, S = A.GENERIC_BIAS2_SPLIT_KV
    _generic(A.select_by_bias(B, H, Nq, Nk, d, S, Nq + S, dtype), dev, f"split k, v {A.IDS[dtype]}", split_kv=True)


def _ragged(c, dev):
    """ops.attention_decode_rows on token-major caches [B, Tmax, H*d] and a q row [B, H*d]"""
    ops = _ops()
    B, H, _, d = c.q.shape
    Tmax = c.k.shape[2]
    q = c.q.permute(0, 2, 1, 3).contiguous().to(dev).permute(0, 2, 1, 3)
    k, v = _pack([c.k, c.v], dev) if d != A.DEC_D else (_pack([c.k], dev)[0], _pack([c.v], dev)[0])
    assert min(c.nk_rows) >= 1 and max(c.nk_rows) <= Tmax
    nk = torch.tensor(c.nk_rows, dtype=torch.int32, device=dev)
    o = Out(B, 1, H, d, c.q.dtype, dev)
    ops.attention_decode_rows(q, k, v, c.scale, nk, out=o.view)
    return o.get()


@pytest.mark.parametrize("dtype", A.HALF, ids=_id)
def test_generic_ragged_rows(dev, dtype):
    """attention_decode_rows at d = 64 falls through to attn_fwd_kernel's nk_rows path: nk_rows = 1, 63, 64, 65, Tmax. The rows past
    nk_rows[b] hold a key that would win (K = 2 k[choice], V = 1000), then NaN: load_tile never forms their address."""
    for nan in (False, True):
        c = A.ragged_poison(A.select_by_qk(5, 3, 1, 130, 64, 20, dtype, nk_rows=A.RAGGED_NK, choice=A.decode_choice(5, 3, A.RAGGED_NK)), nan)
        _exact(_ragged(c, dev), c, f"ragged one-hot nan {nan} {A.IDS[dtype]}")
        c = A.ragged_poison(A.pair_inputs(5, 3, 1, 130, 64, 21, dtype, nk_rows=A.RAGGED_NK, first=64), nan)
        _bounded(_ragged(c, dev), c, A.U16[dtype], "generic", f"ragged pair nan {nan} {A.IDS[dtype]}")


# -------------------------------------------------------------------------------------------------------- ping-pong kernel
@pytest.mark.parametrize("dtype", A.HALF, ids=_id)
def test_pingpong_fp32_tables(dev, dtype):
    """attn_global_pp_kernel<false> (d 80, S 64, k | v fused, Nq 256 and 512): Nk = 64 nkt for nkt = 2 .. 9, every residue of
    (nkt - 1) & 3 and the 4-stage ring twice; the chosen keys include key 0, the last key and key 63 of tile nkt - 2; B * H = 3 and 8.
    Each launch is repeated and has to give the same bits."""
    for B, H, Nq, nkt in A.PP_TABLES:
        c = A.select_by_bias(B, H, Nq, 64 * nkt, 80, 64, Nq + nkt, dtype)
        _bounded(_attention(c, dev, twice=True, pingpong=True), c, A.U16[dtype], "ping-pong", f"bias B {B} H {H} Nq {Nq} nkt {nkt} {A.IDS[dtype]}")


@pytest.mark.parametrize("dtype", A.HALF, ids=_id)
def test_pingpong_pairs(dev, dtype):
    """a in tile 0 and b in the last tile; late_jump: tile 0's best key 40 log2 units below a pair that arrives in tile 1 and the last
    (40 is PP_LAZY in bf16: after rounding about half of the pairs move the lazy reference and half stay on p = 2^40), and 60
    below, which moves it for every pair in both types"""
    for B, H, Nq, nkt, late in A.PP_PAIR:
        c = A.pair_inputs(B, H, Nq, 64 * nkt, 80, Nq + nkt, dtype, late_jump=late, first=64, S=64)
        _bounded(_attention(c, dev, twice=True, pingpong=True), c, A.U16[dtype], "ping-pong", f"pair B {B} H {H} Nq {Nq} nkt {nkt} late {late} {A.IDS[dtype]}")


_T64 = {}


def _tables_64(dtype):
    """select_by_tables_64 at H = 3, built (and its margin asserted) once: q and the tables hold 0 and +-3, exact in both formats"""
    if "c" not in _T64:
        _T64["c"] = A.select_by_tables_64(3, 5, BF16)
    return A.recast_tables_64(_T64["c"], dtype)


def _global(c, dev, H):
    ops = _ops()
    S, d = A.GLB_S, A.GLB_D
    h = A.heads_of(c, H)
    q, k, v = _operands(h, dev)
    th, tw = c.tab_h.float().to(dev), c.tab_w.float().to(dev)
    assert ops.global_attention_supported(q, k, v, S)
    outs = []
    for _ in range(2):
        o = Out(1, S * S, H, d, c.q.dtype, dev)
        ops.global_attention(q, k, v, h.scale, th, tw, S, out=o.view)
        outs.append(o.get())
    assert torch.equal(outs[0], outs[1]), "a second launch gave other bits"
    return outs[0], h


@pytest.mark.parametrize("dtype", A.HALF, ids=_id)
@pytest.mark.parametrize("H", A.PP_FUSED_H)
def test_pingpong_fused_tables(dev, H, dtype):
    """ops.global_attention (N = 4096, B = 1): the bias is computed in the kernel from sign-code tables, k = 0"""
    got, h = _global(_tables_64(dtype), dev, H)
    _bounded(got, h, A.U16[dtype], "ping-pong fused", f"tables H {H} {A.IDS[dtype]}")


@pytest.mark.parametrize("dtype", A.HALF, ids=_id)
def test_pingpong_fused_zero_tables(dev, dtype):
    """q.k selects the key on top of zero tables"""
    S = A.GLB_S
    c = A.select_by_qk(1, 1, S * S, S * S, A.GLB_D, 9, dtype)
    c.tab_h = c.tab_w = torch.zeros((2 * S - 1, A.GLB_D), dtype=dtype)
    got, h = _global(c, dev, 1)
    _bounded(got, h, A.U16[dtype], "ping-pong fused", f"q.k on zero tables {A.IDS[dtype]}")


# ----------------------------------------------------------------------------------------------------------- decode kernels
@pytest.mark.parametrize("dtype", A.HALF, ids=_id)
@pytest.mark.parametrize("shape", A.DECODE, ids=("16waves", "4waves", "1wave"))
def test_decode_rows(dev, shape, dtype):
    """attn_decode_kernel through attention_decode_rows: 16 waves a pair (B * H = 28), 4 waves (224), one wave a head (1053, the last
    workgroup with one live wave); nk_rows on both sides of every 4-, 16-, 64- and 256-key edge. The choice is (7 h + b) % nk, the last
    key for h = 0 and key 0 for h = 1. Rows past nk_rows[b] hold a winning key, then NaN."""
    B, H, Tmax, nks = shape
    for nan in (False, True):
        c = A.decode_case(B, H, Tmax, nks, B + H, dtype, nan=nan)
        _exact(_ragged(c, dev), c, f"decode one-hot B {B} H {H} nan {nan} {A.IDS[dtype]}")
    c = A.decode_case(B, H, Tmax, nks, B + H, dtype, pair=True, nan=True)
    _bounded(_ragged(c, dev), c, A.U32, "decode", f"pair B {B} H {H} {A.IDS[dtype]}")


_ROPE = {}


def _rope_step(dev, shape, dtype):
    """one fused-RoPE decode step per (shape, dtype), shared by the two tests below: -> (Case, qkv_raw, caches before, out, caches after)"""
    key = (shape, dtype)
    if key not in _ROPE:
        ops = _ops()
        B, H, Tmax, nks = shape
        d = A.DEC_D
        c, qkv, k0, v0, cs = A.rope_case(B, H, Tmax, nks, B + H + 1, dtype)
        tok = lambda x: x.permute(0, 2, 1, 3).reshape(B, Tmax, H * d).contiguous()   # noqa: E731
        kc, vc = tok(k0).to(dev), tok(v0).to(dev)
        nk = torch.tensor(nks, dtype=torch.int32, device=dev)
        got = ops.decode_attention_rope(qkv.reshape(B, 3 * H * d).to(dev), kc, vc, cs.to(dev), H, d, c.scale, nk)
        heads = lambda x: x.cpu().view(B, Tmax, H, d).permute(0, 2, 1, 3)   # noqa: E731
        _ROPE[key] = (c, qkv, k0, v0, got.cpu().reshape(B, 1, H, d).permute(0, 2, 1, 3), heads(kc), heads(vc))
    return _ROPE[key]


@pytest.mark.parametrize("dtype", A.HALF, ids=_id)
@pytest.mark.parametrize("shape", A.DECODE, ids=("16waves", "4waves", "1wave"))
def test_decode_rope_fused(dev, shape, dtype):
    """decode_attention_rope with real rotations (theta 10000): q_raw is the inverse rotation of GAIN * kcache[choice] (GAIN * k_new
    where the new row is chosen), so the rotated query picks that key: out == its V row. The appended V row is v_new bit for bit and
    every other cache row of every batch entry keeps its bits (NaN from row nk_rows[b] - 1 on before the step: the kernel may not
    read the row it is about to write)."""
    B, H, Tmax, nks = shape
    c, qkv, k0, v0, got, k1, v1 = _rope_step(dev, shape, dtype)
    _exact(got, c, f"rope B {B} H {H} {A.IDS[dtype]}")
    bits = lambda x: x.contiguous().view(torch.int16)   # noqa: E731
    for b, n in enumerate(nks):
        assert torch.equal(v1[b, :, n - 1], qkv[b, 2]), f"batch {b}: the appended V row is not v_new"
        keep = torch.arange(Tmax) != n - 1
        assert torch.equal(bits(k1[b][:, keep]), bits(k0[b][:, keep])) and torch.equal(bits(v1[b][:, keep]), bits(v0[b][:, keep])), f"batch {b}: a cache row changed"


@pytest.mark.parametrize("dtype", A.HALF, ids=_id)
@pytest.mark.parametrize("shape", A.DECODE, ids=("16waves", "4waves", "1wave"))
def test_decode_rope_appended_k_row(dev, shape, dtype):
    """The appended K row against the float64 rotation of k_new, to one storage ulp.
    With x c -+ x' s formed as two rounded fp32 products and a sum, 1wave-f16 (13 x 81 x 128 = 134 784 elements) stood at 1.51 ulps
    in batch entry 7: the roundings are of the size of the operands (|x| up to 7 here: about 1e-6), and where the two products
    cancel to a result below about 2^-12 of the operands an f16 ulp of that result (f16 keeps 11 bits at every magnitude) is smaller
    than that. The cache kernels (rope8 here, rope_cache_kernel, decode_chain's ch_rope8, held bit-identical to each other) now use
    haff_sum_of_products, one fp32 rounding of the result."""
    B, H, Tmax, nks = shape
    c, _, _, _, _, k1, _ = _rope_step(dev, shape, dtype)
    worst = 0.0
    for b, n in enumerate(nks):
        ulps = (k1[b, :, n - 1].double() - c.k_rot64[b]).abs() / A.ulp(c.k_rot64[b], dtype)
        worst = max(worst, float(ulps.max()))
    print(f"rope appended K row B {B} H {H} {A.IDS[dtype]}: {worst:.3g} storage ulps from the float64 rotation")
    assert worst <= 1.0, f"the appended K row is {worst:.3g} storage ulps off"


# ------------------------------------------------------------------------------------------------------------ window kernel
def _window(c, dev):
    """ops.window_attention on the token-major fused allocation [n_win * N + 1, 3, H, d] whose last row is the pad token and whose
    padded positions hold NaN (they were never written)"""
    ops = _ops()
    n_win, H, N, d = c.q.shape
    holes = c.qkv.clone()
    holes[c.is_pad] = A.NAN
    buf = torch.cat([holes.reshape(n_win * N, 3, H, d), c.pad_row[None]], 0).to(dev)
    q, k, v = (_heads(buf[:-1].view(n_win, N, 3, H, d), i) for i in range(3))
    o = Out(n_win, N, H, d, c.q.dtype, dev)
    ops.window_attention(q, k, v, c.scale, c.tab_h.float().to(dev), c.tab_w.float().to(dev), A.WIN_S, out=o.view, grid=c.grid, pad_token=n_win * N)
    return o.get()


@pytest.mark.parametrize("dtype", A.HALF, ids=_id)
@pytest.mark.parametrize("items", A.WINDOW_ITEMS, ids=lambda t: "%dx%d" % t)
def test_window_items(dev, items, dtype):
    """1, 7, 8, 255, 256, 257 and 270 (window, head) items, every one with its own K / V: past 256 the persistent loop takes a second
    trip out of the other LDS buffer, with odd and even parity. The key is chosen by the in-kernel tables, then by q.k on zero tables."""
    n_win, H = items
    c = A.select_by_tables_14(n_win, H, n_win, dtype)
    _bounded(_window(c, dev), c, A.U16[dtype], "window", f"tables {n_win} x {H} {A.IDS[dtype]}")
    c = A.select_window_qk(n_win, H, n_win, dtype)
    _bounded(_window(c, dev), c, A.U16[dtype], "window", f"q.k {n_win} x {H} {A.IDS[dtype]}")


@pytest.mark.parametrize("dtype", A.HALF, ids=_id)
@pytest.mark.parametrize("grid", A.WINDOW_GRIDS, ids=lambda t: "grid%d-H%d" % t)
def test_window_padded_grids(dev, grid, dtype):
    """two images per launch, the pad row behind the last window: grid 14 (wps 1, no pads, but grid > 0), 15 (edge windows with one
    real row / column, the corner window with a single real token), 20, 28 (wps 2, no pads). Chosen keys include padded positions,
    whose answer is the pad row's V."""
    g, H = grid
    n_win = 2 * (-(-g // A.WIN_S)) ** 2
    for build in (A.select_by_tables_14, A.select_window_qk):
        c = build(n_win, H, g, dtype, g)
        if g % A.WIN_S:
            assert bool(c.is_pad.gather(1, c.choice[:, 0])[~c.is_pad].any()), "no real query chose a padded key"
        _bounded(_window(c, dev), c, A.U16[dtype], "window", f"{build.__name__} grid {g} H {H} {A.IDS[dtype]}")


# -------------------------------------------------------------------------------------------------------------- fp32 kernels
def test_f32_kernels(dev):
    """attn_f32_kernel and the few-keys kernel, ==: (Nq, Nk) = (1, 1), (3, 17), (4, 16), (5, 300) at d 16, 80, 256; causal with q_pos0 = 0
    and Nk - Nq; rel-pos at S 7 and 64 and together with the causal mask; few keys at Nq 256 and 257, Nk 1 and 16, d 16 and 32."""
    for t in A.F32_PLAIN + A.F32_FEW:
        d, B, H, Nq, Nk, causal, p0, _ = t
        c = A.select_by_qk(B, H, Nq, Nk, d, Nq + Nk, F32, bool(causal), p0)
        _exact(_attention(c, dev), c, "f32 qk " + A.case_id(t))
    for t in A.F32_BIAS:
        d, B, H, Nq, Nk, causal, p0, S = t
        c = A.causal_bias_case(d, B, H, Nq, Nk, p0, S, Nq, F32) if causal else A.select_by_bias(B, H, Nq, Nk, d, S, Nq, F32)
        _exact(_attention(c, dev), c, "f32 bias " + A.case_id(t))


def test_f32_ragged_rows(dev):
    """attention_decode_rows in fp32: rows past nk_rows[b] hold a winning key, then NaN"""
    for d, B, H, Tmax, nks in A.F32_RAGGED:
        for nan in (False, True):
            c = A.ragged_poison(A.select_by_qk(B, H, 1, Tmax, d, 20, F32, nk_rows=nks, choice=A.decode_choice(B, H, nks)), nan)
            _exact(_ragged(c, dev), c, f"f32 ragged d {d} nan {nan}")
