"""The backward, loss and optimiser kernels of csrc/train.hip at their edges, each called through its C entry point and compared
on the CPU with the float64 restatement of tests/train_edge_ref.py (checked on its own by tests/test_train_edge_ref_cpu.py).
The bound of every comparison is built there (train_edge_ref.bound / sum_bound): K = 4 times the error the fp32 evaluation of the
same formula shows on the same inputs, a floor of 8 fp32 ulps of the scale, and half an ulp of a 16-bit storage type. Copies and
single roundings are compared with torch.equal. Every output buffer is longer than the kernel's share of it and pre-filled with a
sentinel that has to survive. Each comparison prints its ratio to the bound; the module prints the worst per kernel at the end.

Worst |error| / bound per kernel measured on the MI355X (141 cases, 7.0 s for the file, slowest case 1.7 s): the results stored in
bf16 / f16, where half an ulp of the storage type is nearly the whole bound, reach it — act_fwd 0.999, axpby 1.00, scale_dev
0.996, swiglu fwd / bwd 1.00, norm_bwd dx 1.00, rope 0.999, softmax fwd 0.994 / bwd 0.997, cross_entropy dlogits 0.947; the fp32
results stay well inside — norm_bwd dyx 0.25, cross_entropy loss 0.22, resize_bilinear_bwd 0.25, adamw master 0.23 / m 0.06 / v 0.07,
colsum 0.23 (16-byte 0.09), colsum_partials 0.10, reduce_partials 0.19, sumsq 0.07, sumsq_partials 0.21, mask_loss_stats 0.17
(partials 0.12), mask_loss_grad 0.09 (dev 0.13), scatter_add_rows 0.13 (sorted 0.08), taxonomy_ce 0.16, rope round trip 0.67.
The two forms that end in many atomic adds on one address carry sum_bound's worst-case chain term (1024 adds for mask_loss_stats
at n = 65539, 4096 for sumsq at n = 262149; without it they stood at 9.8 and 1.07): their observed 0.17 and 0.07 are that far below a
bound which, at those two sizes, no longer notices one dropped element. The exact cases there do: +-1 inputs for sumsq and weight 0
for the mask sums give sums that are exact in any order and are compared with ==; the ordered forms keep the tight bound at every n."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_ref as E   # noqa: E402
import train_edge_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu

BAD_ARG = -1
F32, F64, BF16, F16 = R.F32, R.F64, R.BF16, R.F16
_id = lambda v: R.IDS.get(v, None)   # noqa: E731
WORST = {}


def _lib():
    import haff  # noqa: F401
    from haff.lib import load_library
    return load_library()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


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


def _unit(ref):
    """the floor's scale for an elementwise result: its own size, at least 1 (the sigmoid / cdf factor whose error it carries)"""
    return ref.abs().clamp_min(1.0)


class Buf:
    """`n` elements for a kernel to write at an element offset of `off` (0: 256-byte aligned; 1: not even 4-byte aligned for a
    16-bit type) inside a longer sentinel-filled allocation; `init` fills the kernel's share"""

    def __init__(self, n, dtype, dev, off=0, init=None, tail=64):
        self.full = torch.full((off + n + tail,), R.SENT, dtype=dtype, device=dev)
        self.t = self.full[off:off + n]
        self.off, self.n = off, n
        if init is not None:
            self.t.copy_(init.reshape(-1).to(dtype))

    @property
    def ptr(self):
        return self.t.data_ptr()

    def get(self, *shape):
        """the kernel's share on the CPU, after checking that nothing around it was written"""
        full = self.full.cpu()
        assert bool((full[:self.off] == R.SENT).all()) and bool((full[self.off + self.n:] == R.SENT).all()), "written outside the output"
        return full[self.off:self.off + self.n].reshape(*shape) if shape else full[self.off:self.off + self.n]

    def untouched(self):
        return bool((self.full.cpu() == R.SENT).all())


def _inp(x, dev, off=0):
    """x on the device at an element offset inside its allocation"""
    full = torch.zeros((off + x.numel() + 8,), dtype=x.dtype, device=dev)
    full[off:off + x.numel()] = x.reshape(-1)
    return full[off:off + x.numel()]


# ----------------------------------------------------------------------------------------------------------- elementwise
def _elementwise(dev, n, dtype, acts, seed):
    lib, code = _lib(), R.CODE[dtype]
    x, dy = R.edge_values(n, seed, dtype), R.rand((n,), seed + 1).to(dtype)
    xg, dg = x.to(dev), dy.to(dev)
    for act in acts:
        y = Buf(n, dtype, dev)
        assert lib.haff_act_fwd(_p(xg), y.ptr, n, act, code, _s()) == 0
        (ref, bnd), = R.expect(R.act_fwd, x, act, dtypes=(dtype,), scales=(_unit(R.act_fwd(x, act)),))
        _check("act_fwd", y.get(), ref, bnd, f"act {act} n {n} {R.IDS[dtype]}")
        d = Buf(n, dtype, dev)
        assert lib.haff_act_bwd(_p(xg), _p(dg), d.ptr, n, act, code, _s()) == 0
        (ref, bnd), = R.expect(R.act_bwd, x, dy, act, dtypes=(dtype,), scales=(_unit(R.act_bwd(x, dy, act)),))
        got = d.get()
        _check("act_bwd", got, ref, bnd, f"act {act} n {n} {R.IDS[dtype]}")
        if act == R.ACT_RELU:
            assert bool((got[x == 0] == 0).all()), "ReLU's gradient at 0 is 0"
    for b in (dy, None):
        o = Buf(n, dtype, dev)
        assert lib.haff_axpby(_p(xg), _p(dg) if b is not None else None, o.ptr, n, 0.3, -1.7, code, _s()) == 0
        (ref, bnd), = R.expect(R.axpby, x, b, 0.3, -1.7, dtypes=(dtype,))
        _check("axpby", o.get(), ref, bnd, f"b {'set' if b is not None else 'null'} n {n} {R.IDS[dtype]}")
    o = Buf(n, dtype, dev)
    assert lib.haff_mul(_p(xg), _p(dg), o.ptr, n, code, _s()) == 0
    assert torch.equal(o.get(), (x.double() * dy.double()).to(dtype)), "mul is one rounding of an exact product"
    rows = 3 if n % 3 == 0 else 1
    alpha = torch.tensor([0.37, -1.3, 2.5])
    ag = alpha.to(dev)
    for stride in (0, 1):
        o = Buf(n, dtype, dev)
        assert lib.haff_scale_dev(_p(xg), o.ptr, rows, n // rows, _p(ag), stride, code, _s()) == 0
        (ref, bnd), = R.expect(R.scale_rows, x.reshape(rows, -1), alpha, stride, dtypes=(dtype,))
        got = o.get(rows, n // rows)
        _check("scale_dev", got, ref, bnd, f"stride {stride} n {n} {R.IDS[dtype]}")
        if dtype == F32:
            assert torch.equal(got, R.scale_rows(x.reshape(rows, -1), alpha, stride, dt=F32))
    o = Buf(n, dtype, dev)
    assert lib.haff_scale_dev(_p(xg), o.ptr, rows, n // rows, _p(ag), 2, code, _s()) == BAD_ARG
    assert lib.haff_scale_dev(_p(xg), o.ptr, rows, n // rows, None, 0, code, _s()) == BAD_ARG
    torch.cuda.synchronize()
    assert o.untouched()


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_id)
def test_elementwise_edges(dev, dtype):
    """Every activation code and the identity default, +-0 / 1e-3 / 1 / 20 / 100, n of 1, 255 (3 rows of 85 for scale_dev) and 257."""
    for n in R.ELEMENTWISE_N:
        _elementwise(dev, n, dtype, R.ACTS, n)


def test_elementwise_past_the_cap(dev):
    """16384 x 256 + 257 bf16 elements: the grid-stride loops take a second trip"""
    _elementwise(dev, R.ELEMENTWISE_BIG, BF16, (R.ACT_SILU,), 3)


# ---------------------------------------------------------------------------------------------------------------- SwiGLU
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_id)
@pytest.mark.parametrize("Fd", R.SWIGLU_F)
def test_swiglu_both_forms(dev, Fd, dtype):
    """The 16-byte form (aligned pointers) and the scalar form (every pointer one element off) against float64, the same bits from
    both, finite at gates of +-100, nothing written past M * F (M * 2F)."""
    lib, code = _lib(), R.CODE[dtype]
    for M in R.SWIGLU_M:
        gu, dy = R.swiglu_inputs(M, Fd, Fd + M, dtype)
        (rf, bf), = R.expect(R.swiglu_fwd, gu, dtypes=(dtype,), scales=(_unit(R.swiglu_fwd(gu)),))
        (rb, bb), = R.expect(R.swiglu_bwd, gu, dy, dtypes=(dtype,), scales=(_unit(R.swiglu_bwd(gu, dy)),))
        outs = []
        for off in (0, 1):
            gug, dyg = _inp(gu, dev, off), _inp(dy, dev, off)
            y, dgu = Buf(M * Fd, dtype, dev, off), Buf(2 * M * Fd, dtype, dev, off)
            assert (gug.data_ptr() % 16 == 0) == (off == 0)
            assert lib.haff_swiglu_fwd(_p(gug), y.ptr, M, Fd, code, _s()) == 0
            assert lib.haff_swiglu_bwd(_p(gug), _p(dyg), dgu.ptr, M, Fd, code, _s()) == 0
            outs.append((y.get(M, Fd), dgu.get(M, 2 * Fd)))
            assert bool(torch.isfinite(outs[-1][0]).all()) and bool(torch.isfinite(outs[-1][1]).all())
            _check("swiglu_fwd", outs[-1][0], rf, bf, f"M {M} F {Fd} off {off} {R.IDS[dtype]}")
            _check("swiglu_bwd", outs[-1][1], rb, bb, f"M {M} F {Fd} off {off} {R.IDS[dtype]}")
        assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "the two forms differ"


# ------------------------------------------------------------------------------------------------------------- transpose
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_id)
def test_transpose_exact(dev, dtype):
    """[2 x 3][R][ld_in > C] with distinct outer / inner strides -> [6][Cp][Rp], the padding exact zeros"""
    lib = _lib()
    for Rr, C, Rp, Cp, ld in R.TRANSPOSE_CASES:
        base = R.rand((2, 4, Rr + 1, ld), Rr + C).to(dtype)
        out = Buf(6 * Cp * Rp, dtype, dev)
        assert lib.haff_transpose(_p(base.to(dev)), ld, 4 * (Rr + 1) * ld, (Rr + 1) * ld, out.ptr, Rr, C, Rp, Cp, 2, 3, R.CODE[dtype], _s()) == 0
        assert torch.equal(out.get(2, 3, Cp, Rp), R.transpose(base[:, :3, :Rr, :C], Rp, Cp)), (Rr, C, Rp, Cp)


# ----------------------------------------------------------------------------------------------------------------- norms
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_id)
@pytest.mark.parametrize("rms", [0, 1], ids=["ln", "rms"])
def test_norm_adjoints(dev, rms, dtype):
    """Generic kernel at C around 64 and at 4097, the register-resident kernel at 4096 / 5120 and the same rows one element off (the
    generic kernel again); dyx null / set, add absent / present / aliasing dx; a constant row, w with 0 and a negative entry, in
    fp32 a row of mean 100 and spread 1e-2; the row after the last is not written."""
    lib, code = _lib(), R.CODE[dtype]
    eps = R.EPS_RMS if rms else R.EPS_LN
    for rows, C in R.NORM_GENERIC + R.NORM_VEC:
        x, dy, w, add = R.norm_inputs(rows, C, rows + C, dtype)
        wg = w.to(dev)
        for off in ((0, 1) if (rows, C) in R.NORM_VEC else (0,)):
            xg, dg, ag = _inp(x, dev, off), _inp(dy, dev, off), _inp(add, dev, off)
            for mode in ("plain", "add", "alias"):
                a = None if mode == "plain" else add
                (rx, bx), (ry, by) = R.expect(R.norm_bwd, x, dy, w, rms, eps, a, dtypes=(dtype, F32), rowwise=True)
                dx = Buf(rows * C, dtype, dev, off, init=add if mode == "alias" else None)
                dyx = Buf(rows * C, F32, dev, 4 * off) if mode != "add" else None
                if mode == "plain":
                    rc = lib.haff_norm_bwd(_p(xg), _p(dg), _p(wg), dx.ptr, dyx.ptr, rows, C, eps, rms, code, _s())
                else:
                    rc = lib.haff_norm_bwd_add(_p(xg), _p(dg), _p(wg), dx.ptr if mode == "alias" else _p(ag), dx.ptr, dyx.ptr if dyx else None,
                                               rows, C, eps, rms, code, _s())
                assert rc == 0
                what = f"rms {rms} {rows}x{C} off {off} {mode} {R.IDS[dtype]}"
                _check("norm_bwd dx", dx.get(rows, C), rx, bx, what)
                if dyx:
                    _check("norm_bwd dyx", dyx.get(rows, C), ry, by, what)
    o = Buf(8, dtype, dev)
    assert lib.haff_norm_bwd_add(o.ptr, o.ptr, o.ptr, None, o.ptr, None, 1, 8, eps, rms, code, _s()) == BAD_ARG
    assert o.untouched()


# --------------------------------------------------------------------------------------------------------------- softmax
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_id)
@pytest.mark.parametrize("Nk", R.SOFTMAX_NK)
def test_softmax_fwd_and_bwd(dev, Nk, dtype):
    """31 rows of 5 queries (rows % 4 = 3), ld = Nk + 3 with NaN in the padding and in every masked-out score, ldp = Nk + 2 whose
    last two columns are exact zeros; plain and causal at q_pos0 of 0, 3 and Nk - Nq; row 1 has one score 60 above the rest. The
    adjoint reads the rounded P, NaN in dP beyond Nk."""
    lib, code = _lib(), R.CODE[dtype]
    Nq, rows, sc = R.SOFTMAX_NQ, R.SOFTMAX_ROWS, R.SOFTMAX_SCALE
    ld, ldp = Nk + 3, Nk + 2
    for causal, p0 in R.softmax_modes(Nk):
        lim = R.softmax_lim(rows, Nq, Nk, causal, p0)
        s = R.softmax_scores(rows, Nk, ld, lim, Nk + p0)
        (ref, bnd), = R.expect(R.softmax_fwd, s, Nk, ldp, lim, sc, dtypes=(dtype,))
        p = Buf(rows * ldp, dtype, dev)
        assert lib.haff_softmax_fwd(_p(s.to(dev)), ld, p.ptr, ldp, rows, Nq, Nk, sc, causal, p0, code, _s()) == 0
        got = p.get(rows, ldp)
        what = f"Nk {Nk} causal {causal} q_pos0 {p0} {R.IDS[dtype]}"
        _check("softmax_fwd", got, ref, bnd, what)
        j = torch.arange(ldp)[None, :]
        assert bool((got[j.expand(rows, ldp) >= lim[:, None]] == 0).all()), "a masked-out or padding column is not exactly zero"
        live = lim > 0
        assert bool(((got.double().sum(1) - live.double()).abs() <= (bnd * (j < lim[:, None])).sum(1)).all()), "a row does not sum to 1"
        # adjoint, from the P the forward kernel stored
        dp = R.rand((rows, ld), Nk + 7)
        dp[:, Nk:] = R.NAN
        (rd, bd), = R.expect(R.softmax_bwd, got, dp, Nk, ldp, sc, dtypes=(dtype,))
        ds = Buf(rows * ldp, dtype, dev)
        assert lib.haff_softmax_bwd(_p(got.to(dev)), ldp, _p(dp.to(dev)), ld, ds.ptr, rows, Nk, sc, code, _s()) == 0
        gd = ds.get(rows, ldp)
        _check("softmax_bwd", gd, rd, bd, what)
        assert bool((gd[:, Nk:] == 0).all())


# ------------------------------------------------------------------------------------------------------------------ RoPE
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_id)
@pytest.mark.parametrize("d", R.ROPE_D)
def test_rope_forward_and_adjoint(dev, d, dtype):
    """The k slice of a q | k | v row (ldx = 3 H d) into rows of stride H d + 8, at pos0 of 0 and 7; the adjoint of the forward
    returns x to rounding."""
    lib, code = _lib(), R.CODE[dtype]
    H, T, rows = R.ROPE_H, R.ROPE_T, R.ROPE_ROWS
    W = H * d
    for pos0 in R.ROPE_POS0:
        cs = R.rope_table(pos0 + T, d)
        csg = cs.to(dev)
        qkv = R.rand((rows, 3 * W), d + pos0).to(dtype)
        x = qkv[:, W:2 * W]
        qg = qkv.to(dev)
        outs = {}
        for adj in (0, 1):
            (ref, bnd), = R.expect(R.rope, x, cs, T, H, d, pos0, adj, dtypes=(dtype,))
            y = Buf(rows * (W + 8), dtype, dev)
            assert lib.haff_rope(qg.data_ptr() + W * qkv.element_size(), 3 * W, y.ptr, W + 8, _p(csg), rows, T, H, d, pos0, adj, code, _s()) == 0
            got = y.get(rows, W + 8)
            assert bool((got[:, W:] == R.SENT).all()), "columns right of H * d written"
            _check("rope", got[:, :W], ref, bnd, f"d {d} pos0 {pos0} adjoint {adj} {R.IDS[dtype]}")
            outs[adj] = (got[:, :W].contiguous(), bnd)
        yg = outs[0][0].to(dev)
        back = Buf(rows * W, dtype, dev)
        assert lib.haff_rope(_p(yg), W, back.ptr, W, _p(csg), rows, T, H, d, pos0, 1, code, _s()) == 0
        (ref, bnd), = R.expect(R.rope, outs[0][0], cs, T, H, d, pos0, 1, dtypes=(dtype,))
        _check("rope", back.get(rows, W), ref, bnd, f"d {d} pos0 {pos0} adjoint of the forward {R.IDS[dtype]}")
        # ... which is x: the forward's own bound carried through the rotation (at most sqrt(2) of it per element), plus the adjoint's
        _check("rope round trip", back.get(rows, W), x.double(), 2 * outs[0][1].max() + bnd + 4 * R.U32 * x.double().abs().max(), f"d {d} pos0 {pos0} {R.IDS[dtype]}")


# --------------------------------------------------------------------------------------------------------- cross-entropy
def _ce(dev, x, labels, dtype, gscale, what):
    lib, code = _lib(), R.CODE[dtype]
    rows, V = x.shape
    ld = V + 5
    xg = E.widen(x, 5, R.INF).to(dev)
    lg = labels.to(dev)
    sl, sd = R.ce_scales(x, gscale)
    (rl, bl), (rd, bd) = R.expect(R.cross_entropy, x, labels, gscale, dtypes=(F32, dtype), scales=(sl, sd))
    loss, d = Buf(rows, F32, dev), Buf(rows * ld, dtype, dev)
    assert lib.haff_cross_entropy(_p(xg), ld, _p(lg), loss.ptr, d.ptr, rows, V, gscale, code, _s()) == 0
    gl, gd = loss.get(), d.get(rows, ld)
    assert bool((gd[:, V:] == R.SENT).all()), "columns right of V written"
    _check("cross_entropy loss", gl, rl, bl, what)
    _check("cross_entropy dlogits", gd[:, :V], rd, bd, what)
    ign = labels < 0
    assert bool((gl[ign] == 0).all()) and bool((gd[:, :V][ign] == 0).all()), "an ignored row is not exactly zero"
    loss2 = Buf(rows, F32, dev)
    assert lib.haff_cross_entropy(_p(xg), ld, _p(lg), loss2.ptr, None, rows, V, gscale, code, _s()) == 0
    assert torch.equal(loss2.get(), gl), "the loss changes when dlogits is null"


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_id)
@pytest.mark.parametrize("V", R.CE_V)
def test_cross_entropy_edges(dev, V, dtype):
    """Labels 0, V - 1 and -100, a row of equal logits, a logit 30 above the rest at the label and at another column; ld = V + 5 with
    +inf right of V; gscale 0.37; dlogits null."""
    x, labels = R.ce_inputs(V, V, dtype)
    _ce(dev, x, labels, dtype, R.CE_GSCALE, f"V {V} {R.IDS[dtype]}")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_id)
def test_cross_entropy_extreme_rows(dev, dtype):
    """f16 logits of +-65504, fp32 / bf16 logits near -1e4"""
    x, labels = R.ce_extreme(dtype)
    _ce(dev, x, labels, dtype, 1.0, f"extreme {R.IDS[dtype]}")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_id)
def test_cross_entropy_all_ignored_is_zero(dev, dtype):
    """CrossEntropyFn over a batch whose labels are all -100: loss 0 and zero gradient (torch gives NaN)"""
    import haff  # noqa: F401
    from haff import autograd as A
    x = R.rand((4, 37), 1).to(dtype).to(dev).requires_grad_(True)
    loss = A.cross_entropy(x, torch.full((4,), -100, device=dev))
    loss.backward()
    assert float(loss) == 0.0 and bool((x.grad == 0).all())


# ----------------------------------------------------------------------------------------------------------- mask losses
@pytest.mark.parametrize("n", R.MASK_N)
def test_mask_losses(dev, n):
    """Statistics by atomics and by ordered partials (at most 256 per sample), the gradient with host and with device coefficients,
    for weights 1, 0, 2, logits with +-100, targets all 0 / all 1 / mixed; n = 256 * 256 + 3 is past the 256-block cap."""
    lib = _lib()
    x, t = R.mask_inputs(n, n)
    xg, tg = x.to(dev), t.to(dev)
    for wgt in R.MASK_WGT:
        terms = R.mask_terms(x, t, wgt)
        ref = terms.sum(1)
        ev = R.seq_sum32(R.mask_terms(x, t, wgt, dt=F32), 1)
        bnd = R.sum_bound(terms, ev, ref, 1)
        stats = Buf(12, F32, dev, init=torch.zeros(12))
        assert lib.haff_mask_loss_stats(_p(xg), _p(tg), stats.ptr, 3, n, wgt, _s()) == 0
        waves = 4 * min(256, -(-n // 256))          # one atomic add per wave of at most 256 blocks
        _check("mask_loss_stats", stats.get(3, 4), ref, R.sum_bound(terms, ev, ref, 1, chain=waves), f"n {n} w {wgt}")
        if wgt == 0.0:      # p = 0.5 exactly: the three sums are exact in any order, so a dropped element or block shows at any n
            assert torch.equal(stats.get(3, 4)[:, 1:].double(), ref[:, 1:]), "sum(p t), sum(p), sum(t) at weight 0 are not exact"
        parts, n_parts = Buf(3 * 256 * 4, F32, dev), ctypes.c_int(0)
        assert lib.haff_mask_loss_stats_partials(_p(xg), _p(tg), parts.ptr, 3, n, wgt, ctypes.byref(n_parts), _s()) == 0
        assert 0 < n_parts.value <= 256
        out = Buf(12, F32, dev)
        assert lib.haff_reduce_partials(parts.ptr, out.ptr, 12, n_parts.value, 4, 4, n_parts.value * 4, 0, _s()) == 0
        _check("mask_loss_stats_partials", out.get(3, 4), ref, bnd, f"n {n} w {wgt}")
        if wgt == 0.0:
            assert torch.equal(out.get(3, 4)[:, 1:].double(), ref[:, 1:])
        assert bool((parts.full.cpu()[3 * n_parts.value * 4:] == R.SENT).all())
        s32 = ref.float()
        sg = s32.to(dev)
        cb, cd = torch.tensor([2.0, 0.5, 1.0]), torch.tensor([0.5, 1.5, 0.25])
        dx = Buf(3 * n, F32, dev)
        assert lib.haff_mask_loss_grad(_p(xg), _p(tg), _p(sg), dx.ptr, 3, n, wgt, 2.0, 0.5, _s()) == 0
        (rg, bg), = R.expect(R.mask_grad, x, t, s32, wgt, torch.full((3,), 2.0), torch.full((3,), 0.5), rowwise=True)
        _check("mask_loss_grad", dx.get(3, n), rg, bg, f"n {n} w {wgt}")
        dx = Buf(3 * n, F32, dev)
        coef = torch.stack([cb, cd], 1).contiguous().to(dev)
        assert lib.haff_mask_loss_grad_dev(_p(xg), _p(tg), _p(sg), dx.ptr, 3, n, wgt, _p(coef), _s()) == 0
        (rg, bg), = R.expect(R.mask_grad, x, t, s32, wgt, cb, cd, rowwise=True)
        _check("mask_loss_grad_dev", dx.get(3, n), rg, bg, f"n {n} w {wgt}")


# -------------------------------------------------------------------------------------------------------------- taxonomy
@pytest.mark.parametrize("C", R.TAX_C)
def test_taxonomy_ce(dev, C):
    lib = _lib()
    for rows in R.TAX_ROWS:
        for soft in (False, True):
            z, t = R.taxonomy_inputs(rows, C, rows + C, soft)
            zg, tg = z.to(dev), t.to(dev)
            exp = R.expect(R.taxonomy_ce, z, t, dtypes=(F32, F32, F32))
            for with_p, with_dz in ((1, 1), (0, 1), (1, 0)):
                probs, loss, dz = Buf(rows * C, F32, dev), Buf(rows, F32, dev), Buf(rows * C, F32, dev)
                assert lib.haff_taxonomy_ce(_p(zg), _p(tg), probs.ptr if with_p else None, loss.ptr, dz.ptr if with_dz else None, rows, C, _s()) == 0
                what = f"C {C} rows {rows} soft {soft}"
                _check("taxonomy_ce loss", loss.get(), *exp[1], what)
                if with_p:
                    _check("taxonomy_ce probs", probs.get(rows, C), *exp[0], what)
                else:
                    assert probs.untouched()
                if with_dz:
                    _check("taxonomy_ce dz", dz.get(rows, C), *exp[2], what)
                else:
                    assert dz.untouched()


# ------------------------------------------------------------------------------------------------------ bilinear adjoint
@pytest.mark.parametrize("case", E.RESIZE_CASES + (R.RESIZE_BWD_BIG,), ids=lambda c: f"{c[1]}-{c[2]}-{c[3]}")
def test_resize_bilinear_bwd(dev, case):
    """Against the float64 adjoint (no element excluded); pixels outside the crop keep the caller's values; two launches give the
    same bits; <resize(x), g> = <x, resize_bwd(g)> as a second check. The last case is past the 16384-block cap."""
    import haff  # noqa: F401
    from haff import ops
    lib = _lib()
    n, src, crop, out = case
    g = R.rand((n, *out), 5)
    gg = g.to(dev)
    (ref, bnd), = R.expect(R.resize_bwd, g, src, crop)
    gots = []
    for _ in range(2):
        din = Buf(n * src[0] * src[1], F32, dev, init=torch.full((n, *src), 3.5))
        assert lib.haff_resize_bilinear_bwd(_p(gg), din.ptr, n, src[0], src[1], crop[0], crop[1], out[0], out[1], _s()) == 0
        gots.append(din.get(n, *src))
    got = gots[0]
    assert torch.equal(got, gots[1]), "two launches differ"
    inside = torch.zeros(src, dtype=torch.bool)
    inside[:crop[0], :crop[1]] = True
    assert bool((got[:, ~inside] == 3.5).all()), "written outside the crop"
    bnd = bnd[:, inside]
    _check("resize_bilinear_bwd", got[:, inside], ref[:, inside], bnd, str(case))
    if out[0] * 2 < crop[0]:
        assert bool((got[:, inside][ref[:, inside] == 0] == 0).all())
    x = E.resize_source(case, 11, outside=0.0)
    y = ops.resize_bilinear(x.to(dev), crop, out).cpu().double()
    lhs, rhs = (y * g.double()).sum().item(), (x.double()[:, inside] * got.double()[:, inside]).sum().item()
    tol = E.resize_case_tol(x, crop) * g.double().abs().sum().item() + (x.double()[:, inside].abs() * bnd).sum().item()
    print(f"adjoint identity {case}: {lhs:.9g} vs {rhs:.9g}, bound {tol:.3g}")
    assert abs(lhs - rhs) <= tol


# ------------------------------------------------------------------------------------------------------------- scatter
@pytest.mark.parametrize("dtype", R.DTYPES, ids=_id)
@pytest.mark.parametrize("C", R.SCATTER_C)
def test_scatter_add_rows(dev, C, dtype):
    """dE accumulates (pre-filled); ids of -200 / -100 are skipped; every row on one id; ids 0 and V - 1; one row. The sorted form
    adds a run's rows in row order: the same bits as that sum on the CPU, twice."""
    lib, code = _lib(), R.CODE[dtype]
    V = R.SCATTER_V
    for name, ids in R.scatter_ids().items():
        rows = len(ids)
        dx, dE0 = R.rand((rows, C), rows + C).to(dtype), R.rand((V, C), C)
        ref = R.scatter_add(ids, dx, dE0)
        seq = dE0.clone()
        for r, i in enumerate(ids.tolist()):
            if i >= 0:
                seq[i] += dx[r].float()
        # chain = 0 also for the atomic form: an address takes at most 70 adds here (colsum: one per 256 rows, 17 at the most),
        # which the floor covers; sumsq and mask_loss_stats put up to 4096 / 1024 on one address and need the chain term
        bnd = R.sum_bound_abs(seq, ref, R.scatter_abs(ids, dx, dE0))
        dxg = dx.to(dev)
        dE = Buf(V * C, F32, dev, init=dE0)
        assert lib.haff_scatter_add_rows(_p(ids.to(dev)), _p(dxg), dE.ptr, rows, C, code, _s()) == 0
        _check("scatter_add_rows", dE.get(V, C), ref, bnd, f"{name} C {C} {R.IDS[dtype]}")
        sid, order = torch.sort(ids, stable=True)
        for _ in range(2):
            dE = Buf(V * C, F32, dev, init=dE0)
            assert lib.haff_scatter_add_rows_sorted(_p(sid.to(dev)), _p(order.to(dev)), _p(dxg), dE.ptr, rows, C, code, _s()) == 0
            got = dE.get(V, C)
            _check("scatter_add_rows_sorted", got, ref, bnd, f"{name} C {C} {R.IDS[dtype]}")
            assert torch.equal(got, seq), "not the rows of a run added in row order"


# ----------------------------------------------------------------------------------------------------------- reductions
def _colsum(dev, Rr, C, dtype, off, name):
    lib, code = _lib(), R.CODE[dtype]
    x = (R.rand((Rr, C), Rr + C) + 0.3).to(dtype)
    out0 = R.rand((C,), C)
    terms = torch.cat([out0[None].double(), x.double()], 0)
    ref = terms.sum(0)
    bnd = R.sum_bound(terms, R.seq_sum32(terms), ref)
    xg = _inp(x, dev, off)
    out = Buf(C, F32, dev, init=out0)
    assert lib.haff_colsum(_p(xg), out.ptr, Rr, C, code, _s()) == 0
    _check(name, out.get(), ref, bnd, f"{Rr}x{C} off {off} {R.IDS[dtype]}")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_id)
def test_colsum(dev, dtype):
    """The generic kernel at small shapes, the 16-byte kernel at its four widths with row counts that leave a tail (fp32 and an
    8-byte aligned pointer take the generic kernel there); out is added to."""
    for Rr, C in R.COLSUM_GENERIC:
        _colsum(dev, Rr, C, dtype, 0, "colsum generic")
    for Rr, C in R.COLSUM_VEC:
        _colsum(dev, Rr, C, dtype, 0, "colsum generic" if dtype == F32 else "colsum 16-byte")
        if dtype != F32:
            _colsum(dev, Rr, C, dtype, 4, "colsum generic")


@pytest.mark.parametrize("dtype", (F32, BF16), ids=_id)
def test_colsum_partials(dev, dtype):
    lib, code = _lib(), R.CODE[dtype]
    lib.haff_colsum_parts.restype = ctypes.c_int
    C = 5
    assert lib.haff_colsum_parts(0) == 0
    for Rr in R.COLSUM_PARTS_R:
        parts = lib.haff_colsum_parts(Rr)
        assert 1 <= parts <= 256, (Rr, parts)
        x = (R.rand((Rr, C), Rr) + 0.3).to(dtype)
        ref = x.double().sum(0)
        bnd = R.sum_bound(x, R.seq_sum32(x), ref)
        pb = Buf(parts * C, F32, dev)
        assert lib.haff_colsum_partials(_p(x.to(dev)), pb.ptr, Rr, C, code, _s()) == 0
        for acc in (0, 1):
            out = Buf(C, F32, dev, init=torch.full((C,), 2.0))
            assert lib.haff_reduce_partials(pb.ptr, out.ptr, C, parts, C, C, 0, acc, _s()) == 0
            _check("colsum_partials", out.get().double() - 2.0 * acc, ref, bnd + acc * 4 * R.U32 * (ref.abs() + 2.0), f"R {Rr} acc {acc} {R.IDS[dtype]}")
        assert abs(pb.get(parts, C).double().sum(0) - ref).max().item() <= bnd.max().item()


@pytest.mark.parametrize("n_parts", R.REDUCE_PARTS)
def test_reduce_partials(dev, n_parts):
    """two groups of three outputs, parts 3 apart, groups n_parts * 3 + 7 apart with NaN in the gap; overwrite and accumulate"""
    lib = _lib()
    gs = n_parts * 3 + 7
    p = torch.full((2, gs), R.NAN)
    p[:, :n_parts * 3] = R.rand((2, n_parts * 3), n_parts) + 0.2
    terms = p[:, :n_parts * 3].reshape(2, n_parts, 3).double()
    ref = terms.sum(1).reshape(6)
    bnd = R.sum_bound(terms, R.seq_sum32(terms, 1), terms.sum(1), 1).reshape(6)
    pg = p.to(dev)
    for acc in (0, 1):
        out = Buf(6, F32, dev, init=torch.full((6,), 0.5))
        assert lib.haff_reduce_partials(_p(pg), out.ptr, 6, n_parts, 3, 3, gs, acc, _s()) == 0
        _check("reduce_partials", out.get().double() - 0.5 * acc, ref, bnd + acc * 4 * R.U32 * (ref.abs() + 0.5), f"n_parts {n_parts} acc {acc}")


@pytest.mark.parametrize("dtype", R.DTYPES, ids=_id)
def test_sumsq(dev, dtype):
    """Atomic and ordered forms (at most 1024 partials); n = 1024 * 256 + 5 is past the cap; f16 values of 65504; inf gives inf,
    NaN gives NaN."""
    lib, code = _lib(), R.CODE[dtype]
    for n in R.SUMSQ_N:
        for special in (None, "ones", "max", R.INF, R.NAN):
            if special not in (None, "ones") and n not in (257, R.SUMSQ_N[-1]):
                continue
            x = R.rand((n,), n).to(dtype)
            if special == "ones":       # +-1: the sum is n exactly in any order, so a dropped element or block shows at any n
                x = (1.0 - 2.0 * (torch.arange(n) % 2)).to(dtype)
            elif special == "max":
                x[:] = 65504.0
                x = x.to(dtype)
            elif special is not None:
                x[n - 2] = special
            sq = x.double() ** 2
            ref = sq.sum().reshape(1)
            bnd = R.sum_bound(sq, R.seq_sum32(sq), ref)
            if special == R.INF:
                ref = torch.tensor([R.INF], dtype=F64)
            xg = x.to(dev)
            out = Buf(1, F32, dev, init=torch.zeros(1))
            assert lib.haff_sumsq(_p(xg), out.ptr, n, code, _s()) == 0
            waves = 4 * min(1024, -(-n // 256))     # one atomic add per wave of at most 1024 blocks
            atomic = out.get()
            _check("sumsq", atomic, ref, R.sum_bound(sq, R.seq_sum32(sq), ref, chain=waves), f"n {n} {special} {R.IDS[dtype]}")
            pb, n_parts = Buf(1024, F32, dev), ctypes.c_int(0)
            assert lib.haff_sumsq_partials(_p(xg), pb.ptr, n, code, ctypes.byref(n_parts), _s()) == 0
            assert 0 < n_parts.value <= 1024
            out = Buf(1, F32, dev)
            assert lib.haff_reduce_partials(pb.ptr, out.ptr, 1, n_parts.value, 1, 1, 0, 0, _s()) == 0
            _check("sumsq_partials", out.get(), ref, bnd, f"n {n} {special} {R.IDS[dtype]}")
            if special == "ones":
                assert float(out.get()) == float(n) and float(atomic) == float(n), "the sum of n ones is not n"
            assert bool((pb.full.cpu()[n_parts.value:] == R.SENT).all())


# ----------------------------------------------------------------------------------------------------------------- AdamW
def _adamw(dev, n, g_dtype, lp, wd, step, b1, b2, seed):
    lib = _lib()
    w, m, v, g = R.adamw_inputs(n, seed, g_dtype)
    gg = g.to(dev)
    host, devs = 0.5, 0.75
    sc = torch.tensor([devs]).to(dev)
    norm = torch.tensor([3.0]).to(dev)
    lpc = -1 if lp is None else R.CODE[lp]
    res = {}
    for form in ("step", "dev", "skip"):
        mw, mm, mv = Buf(n, F32, dev, init=w), Buf(n, F32, dev, init=m), Buf(n, F32, dev, init=v)
        cp = Buf(n, lp, dev) if lp is not None else None
        head = (mw.ptr, mm.ptr, mv.ptr, _p(gg), cp.ptr if cp else None, n, R.ADAMW_LR, b1, b2, R.ADAMW_EPS, wd, step)
        if form == "step":
            rc = lib.haff_adamw_step(*head, host * devs, R.CODE[g_dtype], lpc, _s())
        elif form == "dev":
            rc = lib.haff_adamw_step_dev(*head, host, _p(sc), R.CODE[g_dtype], lpc, _s())
        else:
            rc = lib.haff_adamw_step_skip(*head, host, _p(sc), _p(norm), R.CODE[g_dtype], lpc, _s())
        assert rc == 0
        res[form] = (mw.get(), mm.get(), mv.get()) + ((cp.get(),) if cp else ())
        if cp:
            assert torch.equal(res[form][3], res[form][0].to(lp)), "the copy is not master rounded once"
    exp = R.expect(R.adamw, w, m, v, g, R.ADAMW_LR, b1, b2, R.ADAMW_EPS, wd, step, host * devs, dtypes=(F32, F32, F32))
    what = f"n {n} g {R.IDS[g_dtype]} wd {wd} step {step} b2 {b2}"
    for form in ("step", "dev"):
        for k, name in enumerate(("master", "m", "v")):
            _check(f"adamw {name}", res[form][k], *exp[k], f"{form} {what}")
    assert all(torch.equal(a, b) for a, b in zip(res["skip"], res["dev"])), "the skip form with a finite norm is not the dev form"
    still = slice(0, None, 97)
    if wd == 0.0:
        assert torch.equal(res["step"][0][still], w[still]), "a zero gradient on zero moments moved the weight"


@pytest.mark.parametrize("lp", (None, BF16, F16), ids=lambda v: R.IDS.get(v, "none"))
@pytest.mark.parametrize("g_dtype", R.DTYPES, ids=_id)
def test_adamw_edges(dev, g_dtype, lp):
    """torch.optim.AdamW in float64: wd 0 / 0.1, step 1 / 2 / 1000, betas (0.9, 0.95) / (0.9, 0.999), n 1 / 257, host scale 0.5 times
    device scale 0.75; the three entry points; the low-precision copy is master.to(dtype)."""
    for n in R.ADAMW_N:
        for wd in (0.0, 0.1):
            for step in (1, 2, 1000):
                for b1, b2 in ((0.9, 0.95), (0.9, 0.999)):
                    _adamw(dev, n, g_dtype, lp, wd, step, b1, b2, n + step)


def test_adamw_past_the_cap(dev):
    _adamw(dev, R.ADAMW_BIG, BF16, BF16, 0.1, 2, 0.9, 0.999, 5)


def test_adamw_skips_on_a_non_finite_norm(dev):
    lib = _lib()
    w, m, v, g = R.adamw_inputs(257, 1, F32)
    for bad in (R.INF, R.NAN):
        bufs = [Buf(257, F32, dev, init=t) for t in (w, m, v)]
        cp = Buf(257, BF16, dev)
        norm = torch.tensor([bad]).to(dev)
        assert lib.haff_adamw_step_skip(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, _p(g.to(dev)), cp.ptr, 257, R.ADAMW_LR, 0.9, 0.95, R.ADAMW_EPS, 0.1, 3,
                                        1.0, None, _p(norm), 1, 0, _s()) == 0
        assert all(torch.equal(b.get(), t) for b, t in zip(bufs, (w, m, v))) and cp.untouched()


# ------------------------------------------------------------------------------------------------------------- refusals
def _refusals(o, a, lab):
    """name -> call; every output pointer lies in the caller's sentinel Buf `o`, every input is `a` (fp32 zeros) or `lab`"""
    lib, s = _lib(), _s()
    return {
        "swiglu_fwd F = 24": lambda: lib.haff_swiglu_fwd(_p(a), o.ptr, 1, 24, 1, s),
        "swiglu_bwd F = 24": lambda: lib.haff_swiglu_bwd(_p(a), _p(a), o.ptr, 1, 24, 1, s),
        "transpose Rp < R": lambda: lib.haff_transpose(_p(a), 4, 16, 16, o.ptr, 4, 4, 3, 4, 1, 1, 1, s),
        "softmax_fwd Nq = 0": lambda: lib.haff_softmax_fwd(_p(a), 8, o.ptr, 8, 4, 0, 8, 1.0, 1, 0, 1, s),
        "softmax_fwd Nq < 0": lambda: lib.haff_softmax_fwd(_p(a), 8, o.ptr, 8, 4, -2, 8, 1.0, 0, 0, 1, s),
        "softmax_fwd ldp < Nk": lambda: lib.haff_softmax_fwd(_p(a), 8, o.ptr, 7, 4, 2, 8, 1.0, 0, 0, 1, s),
        "softmax_bwd ld < Nk": lambda: lib.haff_softmax_bwd(_p(a), 8, _p(a), 7, o.ptr, 4, 8, 1.0, 1, s),
        "softmax_bwd ldp < Nk": lambda: lib.haff_softmax_bwd(_p(a), 7, _p(a), 8, o.ptr, 4, 8, 1.0, 1, s),
        "rope odd d": lambda: lib.haff_rope(_p(a), 9, o.ptr, 9, _p(a), 4, 2, 3, 3, 0, 0, 1, s),
        "rope Tlen = 0": lambda: lib.haff_rope(_p(a), 8, o.ptr, 8, _p(a), 4, 0, 2, 4, 0, 0, 1, s),
        "rope H = 0": lambda: lib.haff_rope(_p(a), 8, o.ptr, 8, _p(a), 4, 2, 0, 4, 0, 0, 1, s),
        "rope d = 0": lambda: lib.haff_rope(_p(a), 8, o.ptr, 8, _p(a), 4, 2, 2, 0, 0, 0, 1, s),
        "rope d < 0": lambda: lib.haff_rope(_p(a), 8, o.ptr, 8, _p(a), 4, 2, 2, -4, 0, 0, 1, s),
        "cross_entropy ld < V": lambda: lib.haff_cross_entropy(_p(a), 7, _p(lab), o.ptr, o.ptr + 64, 4, 8, 1.0, 1, s),
        "taxonomy_ce C = 9": lambda: lib.haff_taxonomy_ce(_p(a), _p(a), o.ptr, o.ptr + 512, o.ptr + 1024, 4, 9, s),
        "resize_bilinear_bwd Ho = 0": lambda: lib.haff_resize_bilinear_bwd(_p(a), o.ptr, 1, 4, 4, 4, 4, 0, 4, s),
        "resize_bilinear_bwd Wo < 0": lambda: lib.haff_resize_bilinear_bwd(_p(a), o.ptr, 1, 4, 4, 4, 4, 4, -1, s),
        "resize_bilinear_bwd Hc > Hs": lambda: lib.haff_resize_bilinear_bwd(_p(a), o.ptr, 1, 4, 4, 5, 4, 4, 4, s),
        "adamw step = 0": lambda: lib.haff_adamw_step(o.ptr, o.ptr + 1024, o.ptr + 2048, _p(a), None, 16, 0.1, 0.9, 0.95, 1e-8, 0.0, 0, 1.0, 1, -1, s),
        "adamw lp_dtype = 1": lambda: lib.haff_adamw_step(o.ptr, o.ptr + 1024, o.ptr + 2048, _p(a), o.ptr + 3072, 16, 0.1, 0.9, 0.95, 1e-8, 0.0, 1, 1.0, 1, 1, s),
        "adamw_dev null scale": lambda: lib.haff_adamw_step_dev(o.ptr, o.ptr + 1024, o.ptr + 2048, _p(a), None, 16, 0.1, 0.9, 0.95, 1e-8, 0.0, 1, 1.0, None, 1, -1, s),
        "adamw_skip null norm": lambda: lib.haff_adamw_step_skip(o.ptr, o.ptr + 1024, o.ptr + 2048, _p(a), None, 16, 0.1, 0.9, 0.95, 1e-8, 0.0, 1, 1.0, None, None, 1, -1, s),
        "act_fwd dtype 2": lambda: lib.haff_act_fwd(_p(a), o.ptr, 16, 0, 2, s),
        "sumsq_partials null count": lambda: lib.haff_sumsq_partials(_p(a), o.ptr, 16, 1, None, s),
        "mask_loss_grad_dev null coef": lambda: lib.haff_mask_loss_grad_dev(_p(a), _p(a), _p(a), o.ptr, 1, 16, 1.0, None, s),
    }


REFUSALS = ("swiglu_fwd F = 24", "swiglu_bwd F = 24", "transpose Rp < R", "softmax_fwd Nq = 0", "softmax_fwd Nq < 0", "softmax_fwd ldp < Nk",
            "softmax_bwd ld < Nk", "softmax_bwd ldp < Nk", "rope odd d", "rope Tlen = 0", "rope H = 0", "rope d = 0", "rope d < 0", "cross_entropy ld < V",
            "taxonomy_ce C = 9", "resize_bilinear_bwd Ho = 0", "resize_bilinear_bwd Wo < 0", "resize_bilinear_bwd Hc > Hs", "adamw step = 0",
            "adamw lp_dtype = 1", "adamw_dev null scale", "adamw_skip null norm", "act_fwd dtype 2", "sumsq_partials null count",
            "mask_loss_grad_dev null coef")


@pytest.mark.parametrize("name", REFUSALS)
def test_refusal_leaves_the_outputs_alone(dev, name):
    """The call returns HAFF_ERR_BAD_ARG before a launch and writes nothing; every buffer is valid for the nearest accepted call."""
    o = Buf(4096, F32, dev)
    a = torch.zeros(4096, device=dev)
    lab = torch.zeros(8, dtype=torch.int64, device=dev)
    calls = _refusals(o, a, lab)
    assert set(calls) == set(REFUSALS)
    rc = calls[name]()
    torch.cuda.synchronize()
    assert rc == BAD_ARG, f"{name}: accepted (return code {rc})"
    assert o.untouched(), f"{name}: an output was written"
    assert bool((a == 0).all()) and bool((lab == 0).all()), f"{name}: an input was written"
