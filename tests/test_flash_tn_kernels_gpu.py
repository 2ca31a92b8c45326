"""The TN weight-gradient product (csrc/gemm_tn.hip) and the flash attention pair (the lse forward of csrc/attention.hip,
csrc/attention_bwd.hip) at their edges, each called through its C entry point and compared on the CPU with the float64 restatements
of tests/flash_tn_ref.py (checked on their own by tests/test_flash_tn_ref_cpu.py). gemm_tn on integer operands, whose every partial
sum is exact in fp32, is compared with ==: one contraction row dropped or counted twice at a slab, split or ragged end moves an entry
by at least 1. The flash pair is held, per output row, to K = 4 times the error of the documented-roundings evaluation, 8 fp32 ulps
of the row's scale, half a storage ulp, and for dq / dk the rounding of delta (flash_tn_ref.delta_terms), on inputs that put a large
share of every causal row on its last visible key; one-hot rows are compared with ==. Every output, lse and workspace sits in a
longer sentinel-filled allocation, the columns between H * 128 and ld included, and the sentinel has to survive; every refusal has
to leave all of them untouched. Each comparison prints its ratio to the bound; the module prints the worst per result at the end.

Measured on the MI355X (56 cases, 5.3 s for the file; pytest --durations=15: test_through_autograd[bf16] 0.86 s, which carries the
first launches, test_gemm_tn_gaussian 0.45 / 0.40 s, test_gemm_tn_exact_rows[bf16] 0.25 s, every other case under 0.1 s). Worst
|error| / bound per result: flash out 0.433, lse2 0.250 (one-hot rows 0.250), dq 0.419, dk 0.212, dv 0.415; gemm_tn f32 0.089,
gemm_tn 16-bit 0.999 (half a storage ulp is nearly the whole of that bound). Every exact gemm_tn case (152 comparisons) has 0
entries that differ. The kernels stand near the blocked CPU evaluation of test_flash_tn_ref_cpu.py (out 0.433, dq 0.302,
dk 0.289, dv 0.285 at its worst): no defect of the mask, q_pos0 or a block end was found. Against the library of the parent commit the same
52 cases pass; the four it cannot pass are the new refusals (test_gemm_tn_new_refusals, test_flash_new_refusals), which that
library would launch, and which were therefore not run on it."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_edge_ref as R   # noqa: E402
import flash_tn_ref as T   # noqa: E402
from test_train_edge_kernels_gpu import Buf   # noqa: E402

pytestmark = pytest.mark.gpu

BAD_ARG, UNSUPPORTED = -1, -2
F32, F64, BF16, F16 = R.F32, R.F64, R.BF16, R.F16
_id = lambda v: T.IDS.get(v, None)   # noqa: E731
WORST = {}
D = T.D


def _lib():
    import haff  # noqa: F401
    from haff.lib import load_library
    return load_library()


def _ag():
    import haff  # noqa: F401
    from haff import autograd
    return autograd


def _s():
    return torch.cuda.current_stream().cuda_stream


def _fn(lib, stem, dtype):
    return getattr(lib, stem + ("_f16" if dtype == F16 else "_bf16"))


def _check(name, got, ref, bnd, what=""):
    r = R.ratio(got, ref, bnd)
    WORST[name] = max(WORST.get(name, 0.0), r)
    print(f"{name} {what}: ratio to bound {r:.3g}")
    assert r <= 1.0, f"{name} {what}: |err| / bound = {r:.3g}"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for name in sorted(WORST):
        print(f"WORST {name}: {WORST[name]:.3g}")


# ------------------------------------------------------------------------------------------------------------------ gemm_tn
def _tn_operand(x, dev, pad_cols=0, col0=0, nan_rows=0):
    """x [M, N] on the device as a view of a wider and longer allocation: `col0` columns before it, `pad_cols` in all beyond its N,
    `nan_rows` rows after row M, every element outside the view NaN"""
    M, N = x.shape
    full = torch.full((M + nan_rows, N + pad_cols), R.NAN, dtype=x.dtype)
    full[:M, col0:col0 + N] = x
    return full.to(dev)[:M, col0:col0 + N]


def _tn(lib, dev, a, b, dtype, out_f32, ag=None, bg=None, twice=True):
    """a^T b through the entry point; -> the result on the CPU. The workspace is exactly haff_gemm_tn_workspace_elems long, out
    exactly N1 * N2, both inside sentinel-filled allocations; a second launch has to give the same bits."""
    M, N1 = a.shape
    N2 = b.shape[1]
    ag = a.to(dev) if ag is None else ag
    bg = b.to(dev) if bg is None else bg
    n_ws = lib.haff_gemm_tn_workspace_elems(M, N1, N2)
    assert n_ws == T.tn_geometry(M, N1, N2)[1] * N1 * N2
    outs = []
    for _ in range(2 if twice else 1):
        ws, out = Buf(n_ws, F32, dev), Buf(N1 * N2, F32 if out_f32 else dtype, dev)
        rc = _fn(lib, "haff_gemm_tn", dtype)(ag.data_ptr(), ag.stride(0), bg.data_ptr(), bg.stride(0), M, N1, N2, ws.ptr, n_ws, out.ptr,
                                             out_f32, _s())
        assert rc == 0, rc
        outs.append(out.get(N1, N2))
        ws.get()     # nothing written around the workspace
    assert len(outs) == 1 or torch.equal(outs[0], outs[1]), "a second launch gave other bits"
    return outs[0]


def _tn_exact(lib, dev, M, N1, N2, dtype, **layout):
    a, b = T.tn_exact_inputs(M, N1, N2, M + N1 + N2, dtype)
    ref = T.gemm_tn(a, b)
    ag, bg = (_tn_operand(a, dev, **layout), _tn_operand(b, dev, **layout)) if layout else (None, None)
    for out_f32 in (1, 0):
        got = _tn(lib, dev, a, b, dtype, out_f32, ag, bg, twice=N1 * N2 < 1 << 20)
        want = ref.float() if out_f32 else ref.to(dtype)      # every entry is an integer below 2^24: one rounding
        bad = int((got != want).sum())
        print(f"gemm_tn exact M {M} N {N1}x{N2} {T.IDS[dtype]} out_f32 {out_f32} {layout}: {bad} entries differ")
        assert torch.equal(got, want), f"M {M} N {N1}x{N2} out_f32 {out_f32}: {bad} entries differ, worst by " \
                                       f"{float((got.double() - want.double()).abs().max())}"


@pytest.mark.parametrize("dtype", T.HALF, ids=_id)
def test_gemm_tn_exact_rows(dev, dtype):
    """Integer operands at every listed contraction length (one row, the slab edge 63 / 64 / 65, the split edge 255 / 256 / 257, the
    64-split cap, a ragged last split of 2.5 slabs) on one cut tile: the fp32 out == the float64 product, the 16-bit out == that
    product rounded once; the short lengths again on a whole tile, 2 x 3 cut tiles and 1 x 16 tiles."""
    lib = _lib()
    for M in T.TN_M:
        _tn_exact(lib, dev, M, 8, 8, dtype)
    for N1, N2 in T.TN_N[1:]:
        for M in T.TN_M_SHORT:
            _tn_exact(lib, dev, M, N1, N2, dtype)
    _tn_exact(lib, dev, 20000, 136, 264, dtype)     # 6 tiles x 63 splits of 320 rows, the last of 160


@pytest.mark.parametrize("dtype", T.HALF, ids=_id)
def test_gemm_tn_reduce_second_sweep(dev, dtype):
    """N1 * N2 = 2048 * 2056 is more than the 4096 x 256 x 4 elements one sweep of gemm_tn_reduce_kernel covers"""
    _tn_exact(_lib(), dev, *T.TN_BIG, dtype)


@pytest.mark.parametrize("dtype", T.HALF, ids=_id)
def test_gemm_tn_layouts(dev, dtype):
    """lda / ldb wider than N with NaN in the padding columns, NaN rows after row M in the allocation, operands that are column slices
    starting 8 and 16 columns in: none of the NaN may reach the result"""
    lib = _lib()
    for M in T.TN_M_SHORT:
        for N1, N2 in ((8, 8), (136, 264)):
            _tn_exact(lib, dev, M, N1, N2, dtype, pad_cols=24, nan_rows=3)
            _tn_exact(lib, dev, M, N1, N2, dtype, pad_cols=24, col0=8)
            _tn_exact(lib, dev, M, N1, N2, dtype, pad_cols=16, col0=16, nan_rows=1)


@pytest.mark.parametrize("dtype", T.HALF, ids=_id)
def test_gemm_tn_gaussian(dev, dtype):
    """Gaussian operands against float64 within sum_bound (chain = 0: the split partials are added in index order) plus half a
    storage ulp"""
    lib = _lib()
    cases = [(M, 8, 8) for M in T.TN_M] + [(M, N1, N2) for N1, N2 in T.TN_N[1:] for M in T.TN_M_SHORT[1:]]
    for M, N1, N2 in cases:
        a, b = T.tn_gauss_inputs(M, N1, N2, M + N1, dtype)
        for out_f32 in (1, 0):
            ref, bnd = T.tn_expect(a, b, F32 if out_f32 else dtype)
            _check("gemm_tn f32" if out_f32 else "gemm_tn 16-bit", _tn(lib, dev, a, b, dtype, out_f32, twice=False), ref, bnd,
                   f"M {M} N {N1}x{N2} {T.IDS[dtype]}")


def _tn_refused(lib, dev, dtype, want, M=65, N1=8, N2=16, lda=8, ldb=16, a_off=0, b_off=0, out_off=0, ws_off=0, ws_short=0, null=()):
    """one refused call: the return code, and out and the workspace untouched. *_off: bytes added to a base pointer"""
    a, b = T.tn_exact_inputs(65, 16, 24, 1, dtype)
    ag, bg = a.to(dev), b.to(dev)
    n_ws = 4096
    ws, out = Buf(n_ws, F32, dev), Buf(1024, F32, dev)
    ptr = {"a": ag.data_ptr() + a_off, "b": bg.data_ptr() + b_off, "ws": ws.ptr + ws_off, "out": out.ptr + out_off}
    for name in null:
        ptr[name] = None
    for out_f32 in (0, 1):
        rc = _fn(lib, "haff_gemm_tn", dtype)(ptr["a"], lda, ptr["b"], ldb, M, N1, N2, ptr["ws"], n_ws - ws_short, ptr["out"], out_f32, _s())
        assert rc == want, (rc, want)
    torch.cuda.synchronize()
    assert ws.untouched() and out.untouched()


@pytest.mark.parametrize("dtype", T.HALF, ids=_id)
def test_gemm_tn_workspace_and_refusals(dev, dtype):
    """A workspace of exactly haff_gemm_tn_workspace_elems is accepted (every passing case above) and one element fewer refused; sizes
    <= 0, null pointers, lda < N1, N or ld not a multiple of 8, bases 2 bytes off, and a count past an int are refused, out and the
    workspace untouched."""
    lib = _lib()
    a, b = T.tn_exact_inputs(257, 8, 16, 2, dtype)
    ag, bg = a.to(dev), b.to(dev)
    n_ws = lib.haff_gemm_tn_workspace_elems(257, 8, 16)
    assert n_ws == 2 * 8 * 16
    ws, out = Buf(n_ws, F32, dev), Buf(8 * 16, F32, dev)
    assert _fn(lib, "haff_gemm_tn", dtype)(ag.data_ptr(), 8, bg.data_ptr(), 16, 257, 8, 16, ws.ptr, n_ws - 1, out.ptr, 1, _s()) == BAD_ARG
    torch.cuda.synchronize()
    assert ws.untouched() and out.untouched()
    assert _fn(lib, "haff_gemm_tn", dtype)(ag.data_ptr(), 8, bg.data_ptr(), 16, 257, 8, 16, ws.ptr, n_ws, out.ptr, 1, _s()) == 0
    assert torch.equal(out.get(8, 16).double(), T.gemm_tn(a, b))
    for kw in (dict(M=0), dict(M=-1), dict(N1=0), dict(N2=0), dict(N1=-8), dict(null=("a",)), dict(null=("b",)), dict(null=("ws",)),
               dict(null=("out",)), dict(lda=0), dict(N1=16, lda=8), dict(N2=24, ldb=16)):
        _tn_refused(lib, dev, dtype, BAD_ARG, **kw)
    for kw in (dict(N1=4, lda=8), dict(N2=12), dict(lda=12), dict(ldb=20), dict(a_off=2), dict(b_off=2), dict(out_off=2), dict(a_off=8)):
        _tn_refused(lib, dev, dtype, UNSUPPORTED, **kw)
    for args, want in (((0, 8, 8), BAD_ARG), ((8, 0, 8), BAD_ARG), ((8, 8, -8), BAD_ARG), ((64, 65536, 65536), UNSUPPORTED),
                       ((1 << 20, 65536, 32768), UNSUPPORTED), ((64, 32768, 32768), 1 << 30)):
        assert lib.haff_gemm_tn_workspace_elems(*args) == want, args


@pytest.mark.parametrize("dtype", T.HALF, ids=_id)
def test_gemm_tn_new_refusals(dev, dtype):
    """a workspace that is not 16-byte aligned (the partials move 16 bytes at a time) is refused before any launch"""
    lib = _lib()
    for off in (4, 8, 12):
        _tn_refused(lib, dev, dtype, BAD_ARG, ws_off=off, ws_short=4)


# --------------------------------------------------------------------------------------------------------------- flash pair
class Flash:
    """One problem of the pair on the device: token-major operands [B][N][ld] with NaN in the columns past H * 128, every result in
    its own sentinel-filled Buf; the workspace is exactly the header's roundup(B*H*Nq, 4) + B*H*128*roundup(Nq, 64) values."""

    def __init__(self, dev, inputs, shape, dtype):
        self.B, self.H, self.Nq, self.Nk, self.causal, self.q_pos0, extra = shape
        self.ld = self.H * D + extra
        self.dev, self.dtype = dev, dtype
        self.q, self.k, self.v, self.do = (T.to_token_major(t.to(dtype), self.ld).to(dev) for t in inputs)
        B, H, Nq, Nk = self.B, self.H, self.Nq, self.Nk
        self.n_ws = T.bwd_workspace_elems(B, H, Nq)
        self.out, self.lse = Buf(B * Nq * self.ld, dtype, dev), Buf(B * H * Nq, F32, dev)
        self.new_grads()

    def new_grads(self):
        B, Nq, Nk, ld = self.B, self.Nq, self.Nk, self.ld
        self.dq, self.dk, self.dv = Buf(B * Nq * ld, self.dtype, self.dev), Buf(B * Nk * ld, self.dtype, self.dev), Buf(B * Nk * ld, self.dtype, self.dev)
        self.ws = Buf(self.n_ws, F32, self.dev)

    def fwd(self, lib, **o):
        """the lse entry point; `o` overrides arguments: q / k / v / out / lse pointers, B, H, Nq, Nk, d, ld, causal, q_pos0"""
        g = lambda n, dflt: o[n] if n in o else dflt   # noqa: E731
        ld, Nq, Nk = g("ld", self.ld), g("Nq", self.Nq), g("Nk", self.Nk)
        return _fn(lib, "haff_attention_lse", self.dtype)(
            g("q", self.q.data_ptr()), Nq * ld, D, ld, g("k", self.k.data_ptr()), Nk * ld, D, ld, g("v", self.v.data_ptr()), Nk * ld, D, ld,
            g("out", self.out.ptr), Nq * ld, D, ld, g("B", self.B), g("H", self.H), Nq, Nk, g("d", D), T.FLASH_SCALE, g("causal", self.causal),
            g("q_pos0", self.q_pos0), g("lse", self.lse.ptr), _s())

    def bwd(self, lib, **o):
        g = lambda n, dflt: o[n] if n in o else dflt   # noqa: E731
        return _fn(lib, "haff_attention_bwd", self.dtype)(
            g("q", self.q.data_ptr()), g("k", self.k.data_ptr()), g("v", self.v.data_ptr()), g("out", self.out.ptr), g("do", self.do.data_ptr()),
            g("lse", self.lse.ptr), g("dq", self.dq.ptr), g("dk", self.dk.ptr), g("dv", self.dv.ptr), g("ws", self.ws.ptr),
            g("n_ws", self.n_ws), g("ld", self.ld), g("B", self.B), g("H", self.H), g("Nq", self.Nq), g("Nk", self.Nk), g("d", D),
            T.FLASH_SCALE, g("causal", self.causal), g("q_pos0", self.q_pos0), _s())

    def _heads(self, buf, N):
        """[B, H, N, 128] on the CPU; the columns past H * 128 must still hold the sentinel (Buf.get checks around the buffer)"""
        t = buf.get(self.B, N, self.ld)
        assert bool((t[:, :, self.H * D:] == R.SENT).all()), "the columns between H * 128 and ld were written"
        return T.from_token_major(t, self.H)

    def results(self):
        """out, lse2, dq, dk, dv as flash_tn_ref.attn returns them"""
        self.ws.get()
        return (self._heads(self.out, self.Nq), self.lse.get(self.B, self.H, self.Nq), self._heads(self.dq, self.Nq),
                self._heads(self.dk, self.Nk), self._heads(self.dv, self.Nk))

    def run(self, lib):
        """forward, then the backward fed with the out and lse the forward wrote, as the trainer does"""
        assert self.fwd(lib) == 0
        assert self.bwd(lib) == 0
        return self.results()

    def untouched(self):
        torch.cuda.synchronize()
        return all(b.untouched() for b in (self.out, self.lse, self.dq, self.dk, self.dv, self.ws))


def _mask(shape):
    return shape[4], shape[5]


@pytest.mark.parametrize("dtype", T.HALF, ids=_id)
@pytest.mark.parametrize("shape", T.FLASH_SHAPES, ids=T.flash_id)
def test_flash_pair_on_the_trap(dev, shape, dtype):
    """Trap inputs (every causal row's last visible key, and the first masked one, carry a large share) at every listed shape: out, lse2,
    dq, dk, dv against float64 within the per-row bound; keys no query sees get dk and dv rows of exactly zero."""
    B, H, Nq, Nk, causal, q_pos0, _ = shape
    inputs = T.trap_inputs(B, H, Nq, Nk, q_pos0, Nq + Nk, dtype)
    got = Flash(dev, inputs, shape, dtype).run(_lib())
    exp = T.attn_expect(*inputs, T.FLASH_SCALE, causal, q_pos0, dtype)
    fails = []
    for name, g, (ref, bnd) in zip(T.RESULTS, got, exp):
        try:
            _check(f"flash {name}", g, ref, bnd, f"{T.flash_id(shape)} {T.IDS[dtype]}")
        except AssertionError as e:
            fails.append(str(e))
    assert not fails, fails
    unseen = T.unseen_keys(Nq, Nk, causal, q_pos0)
    assert bool((got[3][:, :, unseen] == 0).all()) and bool((got[4][:, :, unseen] == 0).all()), "dk / dv of a key no query sees"


ONEHOT_SHAPES = ((1, 1, 330, 333, 1, 3, 0), (1, 2, 70, 133, 1, 63, 64), (1, 1, 130, 70, 0, 0, 0), (1, 1, 65, 65, 1, 0, 0), (1, 3, 129, 129, 1, 0, 64))


@pytest.mark.parametrize("dtype", T.HALF, ids=_id)
def test_flash_pair_one_hot(dev, dtype):
    """Every query's chosen key (0, 63, 64, 127, 128, the last one, the causal diagonal) scores 160 log2 units above the other visible
    keys, so every other probability is exactly 0 in fp32: out == the chosen V row, dv == the scatter-sum of the integer dO rows by
    choice, lse2 within the bound of the chosen score."""
    lib = _lib()
    for shape in ONEHOT_SHAPES:
        B, H, Nq, Nk, causal, q_pos0, _ = shape
        q, k, v, do, choice = T.onehot_inputs(B, H, Nq, Nk, causal, q_pos0, Nq, dtype)
        out, lse2, _, _, dv = Flash(dev, (q, k, v, do), shape, dtype).run(lib)
        what = f"{T.flash_id(shape)} {T.IDS[dtype]}"
        bad = (out != v[:, :, choice]).any(-1)
        assert not bool(bad.any()), f"{what}: out is not the chosen V row at queries {bad.nonzero()[:8].tolist()} (choices {choice[bad[0, 0]][:8].tolist()})"
        scatter = torch.zeros((B, H, Nk, D), dtype=F64).index_add_(2, choice, do.double())
        bad = (dv.double() != scatter).any(-1)
        assert not bool(bad.any()), f"{what}: dv is not the scatter-sum of dO at keys {bad.nonzero()[:8].tolist()}"
        ref, bnd = T.attn_expect(q, k, v, do, T.FLASH_SCALE, causal, q_pos0, dtype)[1]
        _check("flash lse2 one-hot", lse2, ref, bnd, what)


def _single_head(lib, dev, full, b, h):
    """head (b, h) of `full` run alone: B = H = 1, the same ld, the operands read in place"""
    one = Flash(dev, [torch.zeros((1, 1, 1, D))] * 4, (1, 1, full.Nq, full.Nk, full.causal, full.q_pos0, full.ld - D), full.dtype)
    assert one.ld == full.ld
    at = lambda t, N: t.data_ptr() + ((b * N * full.ld) + h * D) * 2   # noqa: E731
    ptrs = dict(q=at(full.q, full.Nq), k=at(full.k, full.Nk), v=at(full.v, full.Nk))
    assert one.fwd(lib, **ptrs) == 0
    assert one.bwd(lib, do=at(full.do, full.Nq), **ptrs) == 0
    return one.results()


@pytest.mark.parametrize("dtype", T.HALF, ids=_id)
def test_flash_heads_alone_repeat_and_scaling(dev, dtype):
    """Smooth inputs, B * H = 16, Nq = Nk = 300, ld = H * 128 + 64. Each (b, h) is bit-equal, forward and backward, to the same head run
    alone with B = H = 1 and the same ld; a second backward gives the same bits; dO * 2^8 gives exactly 2^8 times dq, dk, dv in bf16
    (every step of the backward is linear in dO, scaling by a power of two is exact in fp32, and bf16 has fp32's exponent range).
    f16 is held to the per-row bound instead: dS = P (dP - delta) scale has values in f16's subnormal range, whose rounding step
    does not scale with the value, so there the scaling is not exact."""
    lib = _lib()
    shape = (2, 8, 300, 300, 1, 0, 64)
    B, H, Nq, Nk, causal, q_pos0, _ = shape
    inputs = T.smooth_inputs(B, H, Nq, Nk, 11, dtype)
    full = Flash(dev, inputs, shape, dtype)
    got = full.run(lib)
    for b in range(B):
        for h in range(H):
            for name, g, o in zip(T.RESULTS, got, _single_head(lib, dev, full, b, h)):
                assert torch.equal(g[b, h], o[0, 0]), f"{name} of head ({b}, {h}) differs from the head run alone"
    full.new_grads()
    assert full.bwd(lib) == 0
    again = full.results()
    for name, g, o in zip(T.RESULTS[2:], got[2:], again[2:]):
        assert torch.equal(g, o), f"{name}: a second backward gave other bits"
    scaled = (inputs[3].float() * 256.0).to(dtype)
    assert torch.equal(scaled.float(), inputs[3].float() * 256.0)
    full.do = T.to_token_major(scaled, full.ld).to(dev)
    full.new_grads()
    assert full.bwd(lib) == 0
    big = full.results()
    if dtype == BF16:
        for name, g, o in zip(T.RESULTS[2:], got[2:], big[2:]):
            assert torch.equal(g.float() * 256.0, o.float()), f"{name}: dO * 2^8 did not give 2^8 times the gradient"
    else:
        exp = T.attn_expect(inputs[0], inputs[1], inputs[2], scaled, T.FLASH_SCALE, causal, q_pos0, dtype)
        for name, g, (ref, bnd) in list(zip(T.RESULTS, big, exp))[2:]:
            _check(f"flash {name}", g, ref, bnd, f"dO * 2^8 {T.flash_id(shape)} f16")


def _flash_problem(dev, dtype, shape=(1, 3, 129, 129, 1, 0, 64)):
    B, H, Nq, Nk, causal, q_pos0, _ = shape
    return Flash(dev, T.smooth_inputs(B, H, Nq, Nk, 5, dtype), shape, dtype)


@pytest.mark.parametrize("dtype", T.HALF, ids=_id)
def test_flash_bwd_workspace_edge(dev, dtype):
    """B * H * Nq = 387 is no multiple of 4: the header's roundup(B*H*Nq, 4) + B*H*128*roundup(Nq, 64) values are accepted (every passing
    case above runs on exactly that many), one value fewer is refused, and so is a workspace 4 bytes off"""
    lib = _lib()
    f = _flash_problem(dev, dtype)
    assert f.n_ws == 388 + 3 * 128 * 192
    assert f.fwd(lib) == 0
    torch.cuda.synchronize()
    assert f.bwd(lib, n_ws=f.n_ws - 1) == BAD_ARG
    assert f.bwd(lib, ws=f.ws.ptr + 4) == BAD_ARG
    torch.cuda.synchronize()
    assert all(b.untouched() for b in (f.dq, f.dk, f.dv, f.ws))
    assert f.bwd(lib) == 0
    f.results()


@pytest.mark.parametrize("dtype", T.HALF, ids=_id)
def test_flash_refusals(dev, dtype):
    """Refused before any launch, outputs, lse and workspace untouched: d != 128 for the backward, ld < H * 128 or no multiple of 8, bases
    2 or 8 bytes off and null pointers for the backward, sizes <= 0, a null lse"""
    lib = _lib()
    f = _flash_problem(dev, dtype)
    assert f.bwd(lib, d=64) == UNSUPPORTED and f.bwd(lib, d=136) == UNSUPPORTED
    for kw in (dict(ld=f.H * D - 8), dict(ld=f.H * D + 4), dict(B=0), dict(H=0), dict(Nq=0), dict(Nk=0), dict(B=-1), dict(Nq=-5), dict(lse=None)):
        assert f.bwd(lib, **kw) == BAD_ARG, kw
        if kw.get("ld", f.ld) >= f.H * D:      # the forward takes general strides: a short ld is the backward's refusal alone
            assert f.fwd(lib, **kw) == BAD_ARG, kw
    for name in ("q", "k", "v", "out", "do", "dq", "dk", "dv"):
        base = getattr(f, name)
        base = base.ptr if isinstance(base, Buf) else base.data_ptr()
        for p in (None, base + 2, base + 8):
            assert f.bwd(lib, **{name: p}) == BAD_ARG, (name, p)
    assert f.bwd(lib, ws=None) == BAD_ARG
    assert f.untouched()


@pytest.mark.parametrize("dtype", T.HALF, ids=_id)
def test_flash_new_refusals(dev, dtype):
    """causal with q_pos0 = -1 and -64 (a query row without a visible key has no log-sum-exp; with q_pos0 <= -64 the backward's key
    block 0 skips query block 0, whose fp32 dq sums would then never be written) is refused by all four entry points; the lse
    entry points refuse null q / k / v / o and bases their 16-byte loads (8-byte stores for o) cannot take"""
    lib = _lib()
    f = _flash_problem(dev, dtype)
    for q_pos0 in (-1, -64):
        assert f.fwd(lib, causal=1, q_pos0=q_pos0) == BAD_ARG
        assert f.bwd(lib, causal=1, q_pos0=q_pos0) == BAD_ARG
    for name in ("q", "k", "v"):
        for p in (None, getattr(f, name).data_ptr() + 2, getattr(f, name).data_ptr() + 8):
            assert f.fwd(lib, **{name: p}) == BAD_ARG, (name, p)
    for p in (None, f.out.ptr + 2, f.out.ptr + 4):
        assert f.fwd(lib, out=p) == BAD_ARG, p
    assert f.fwd(lib, lse=f.lse.ptr + 2) == BAD_ARG
    assert f.untouched()


# ------------------------------------------------------------------------------------------------------------- through Python
@pytest.mark.parametrize("dtype", T.HALF, ids=_id)
def test_through_autograd(dev, dtype):
    """FlashAttentionFn (its workspace arithmetic and q_pos0 = Nk - Nq) at the 70 x 133 trap shape and LinearFn's TN route for dW at
    257 x (136, 264), within the same bounds"""
    A = _ag()
    B, H, Nq, Nk, causal = 1, 2, 70, 133, 1
    inputs = T.trap_inputs(B, H, Nq, Nk, Nk - Nq, Nq + Nk, dtype)
    q, k, v, do = (T.to_token_major(t, H * D).to(dev) for t in inputs)
    q, k, v = (t.requires_grad_(True) for t in (q, k, v))
    assert A.FLASH_TRAINING_ATTENTION
    o = A.attention(q, k, v, H, T.FLASH_SCALE, True)
    assert "Flash" in type(o.grad_fn).__name__
    o.backward(do)
    exp = T.attn_expect(*inputs, T.FLASH_SCALE, causal, Nk - Nq, dtype)
    for name, g in (("out", o.detach()), ("dq", q.grad), ("dk", k.grad), ("dv", v.grad)):
        ref, bnd = exp[T.RESULTS.index(name)]
        _check(f"flash {name}", T.from_token_major(g.cpu(), H), ref, bnd, f"FlashAttentionFn {T.IDS[dtype]}")
    M, N, K = 257, 136, 264
    gy, x = T.tn_gauss_inputs(M, N, K, 7, dtype)
    xg = x.to(dev).requires_grad_(True)
    w = (R.rand((N, K), 9) * K ** -0.5).to(dtype).to(dev).requires_grad_(True)
    assert A.TN_WEIGHT_GRADIENTS and A.gemm_tn_supported(gy.to(dev), xg.detach())
    A.linear(xg, w).backward(gy.to(dev))
    ref, bnd = T.tn_expect(gy, x, dtype)
    _check("gemm_tn 16-bit", w.grad.cpu(), ref, bnd, f"LinearFn dW {T.IDS[dtype]}")
