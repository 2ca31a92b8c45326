"""The 16-bit GEMM family (csrc/gemm_bf16.hip) on operands whose exact result is known (tests/gemm_edge_ref.py, checked on its own by
tests/test_gemm_edge_ref_cpu.py), one case per dispatch branch of gemm_bf16_impl, launch_skinny and launch_skinny_splitk: every case
names its branch and the Python mirror of the dispatcher must agree before anything is launched.

Integer (or power-of-two scaled) operands keep every partial sum exact in fp32 in ANY summation order, so products, biases, residuals,
row maps, gathers, folded norms with power-of-two statistics, the head-major scatter, RoPE with cos / sin in {0, +-1, +-1/2}, the
{sum, sum of squares} partials and the batched strides are compared with ==: fp32 outputs against the exact value, 16-bit outputs against
torch's round-to-nearest-even conversion of it. Only GELU, quick-GELU, SiLU and SwiGLU are bounded (gemm_edge_ref.bound: numbers from the
formats and the arithmetic): an fp32 output within b of the float64 result, a 16-bit output inside [to16(ref - b), to16(ref + b)].

Every output goes through out= into a NaN-filled allocation with a guard row above and below and guard columns behind every row: 64
of them (a 16-byte aligned C with ldc % 8 == 0, what the specialised instances need) and, in a second variant, 3 (an odd pitch: the
element-store paths). Guards, dropped rows and unmapped rows must keep their bits. Operand rows sit in NaN-padded allocations (pitch
K + 8), so a chunk read behind a row's end shows. References are float64 on the device; only mismatch counts and worst ratios come
back to the host. Every case is a geometry its entry point admits; nothing here is meant to fault."""
import functools
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_edge_ref as G   # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F16, F32, F64 = G.BF16, G.F16, G.F32, G.F64
WORST = {}       # name -> worst |err| / bound of the bounded cases
LAUNCHED = {}    # test -> the specialised instances its launches met the contract of: PREDICTED by gemm_edge_ref.spec_instance, a
                 # restatement of launch_gemm's choice (the library does not report the instance it ran)
_dt = lambda d: {BF16: "bf16", F16: "f16", F32: "f32"}[d]   # noqa: E731


def _ops():
    import haff  # noqa: F401
    from haff import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for name in sorted(WORST):
        print(f"WORST {name}: {WORST[name]:.3g} of the bound")
    for name in sorted(LAUNCHED):
        print(f"SPEC (predicted) {name}: {sorted(LAUNCHED[name])}")


# ------------------------------------------------------------------------------------------------------------- allocations
def _ints_of(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


def _bad(big, exp):
    """elements of a whole allocation that differ from what is expected of them: exp NaN = the sentinel's bits must still be there"""
    sent = _ints_of(torch.full((1,), G.NAN, dtype=big.dtype, device=big.device))
    return torch.where(torch.isnan(exp), _ints_of(big) != sent, big != exp)


class Out:
    """the out= argument [rows, cols] as a view of a NaN-filled [rows + 2, cols + guard] allocation"""

    def __init__(self, rows, cols, dtype, dev, guard):
        self.rows, self.cols = rows, cols
        self.big = torch.full((rows + 2, cols + guard), G.NAN, dtype=dtype, device=dev)
        self.view = self.big[1:rows + 1, :cols]

    def expected(self, want):
        exp = torch.full_like(self.big, G.NAN)
        exp[1:self.rows + 1, :self.cols] = want
        return exp

    def check(self, want, what):
        """== everywhere: values where want holds one, the sentinel where want is NaN and in every guard"""
        bad = _bad(self.big, self.expected(want))
        n = int(bad.sum())
        if n:
            at = bad.nonzero()[:6]
            got = [(int(i) - 1, int(j), float(self.big[i, j])) for i, j in at.tolist()]
            raise AssertionError(f"{what}: {n} of {bad.numel()} elements differ (guards included); (row, col, got) {got}, "
                                 f"want {[float(want[min(max(i, 0), self.rows - 1), min(j, self.cols - 1)]) for i, j, _ in got]}")

    def guards_kept(self, what):
        exp = self.expected(torch.zeros((self.rows, self.cols), dtype=self.big.dtype, device=self.big.device))
        keep = torch.isnan(exp)
        n = int((_bad(self.big, exp) & keep).sum())
        assert n == 0, f"{what}: {n} guard elements were written"


def _operand(t64, dtype, dev):
    """[rows, K] of a 16-bit operand as a view of a NaN-padded [rows, K + 8] allocation (16-byte aligned rows)"""
    rows, K = t64.shape
    big = torch.full((rows, K + 8), G.NAN, dtype=dtype, device=dev)
    big[:, :K] = t64.to(dev)
    return big[:, :K]


def _f32(t, dev):
    return None if t is None else t.float().contiguous().to(dev)


# ------------------------------------------------------------------------------------------------------------------- cases
class Case:
    """one product: 16-bit operands on the device, the float64 gathered product, and check(): a launch of ops.linear with one
    epilogue into a guarded allocation, compared with gemm_edge_ref.gemm_ref"""

    def __init__(self, dev, dtype, a, w, mirror, test, bias=None, a_map=None, ln_stats=None, ln_colsum=None):
        self.dev, self.dtype, self.mirror, self.test = dev, dtype, mirror, test
        assert G.is16(a, dtype) and G.is16(w, dtype)
        self.x, self.wt = _operand(a, dtype, dev), _operand(w, dtype, dev)
        self.N = w.shape[0]
        self.bias64 = None if bias is None else bias.to(dev)
        self.a_map = None if a_map is None else a_map.to(dev)
        self.st64 = None if ln_stats is None else ln_stats.to(dev)
        self.cs64 = None if ln_colsum is None else ln_colsum.to(dev)
        a64, w64 = a.to(dev), w.to(dev)
        self.acc = (a64 if a_map is None else a64[self.a_map.long()]) @ w64.T
        self.M = self.acc.shape[0]
        self.bias, self.ln_stats, self.ln_colsum = _f32(bias, dev), _f32(ln_stats, dev), _f32(ln_colsum, dev)

    def launch(self, cfg, guard, out_dtype, act=0, resid=None, row_map=None, rows=None, inplace=False, swiglu=False, bias=True):
        """-> (the guarded output, the float64 reference [rows, n_out] with NaN where nothing may be written, the pre-activation)"""
        ops = _ops()
        dev = self.dev
        n_out = self.N // 2 if swiglu else self.N
        rows = self.M if rows is None else rows
        o = Out(rows, n_out, out_dtype, dev, guard)
        prefill = torch.full((rows, n_out), G.NAN, dtype=F64, device=dev)
        r = r64 = None
        if resid is not None:
            r64 = resid.to(dev)
            if inplace:
                o.view.copy_(r64)
                r, prefill = o.view, r64
            else:
                r = r64.to(out_dtype).contiguous()
        rm = None if row_map is None else row_map.to(dev)
        b64 = self.bias64 if bias else None
        ops.linear(self.x, self.wt, bias=self.bias if bias else None, act=act, resid=r, row_map=rm, out=o.view, tile_cfg=cfg,
                   swiglu=swiglu, a_map=self.a_map, ln_stats=self.ln_stats, ln_colsum=self.ln_colsum)
        spec = G.spec_instance(self.mirror, self.M, self.N, o.view.stride(0), out_dtype == F32, bias=bias and b64 is not None,
                               ln=self.st64 is not None, csum=self.cs64 is not None, res=r is not None,
                               ldr=0 if r is None else r.stride(0), row_map=rm is not None, act=act, swiglu=swiglu)
        if spec:
            LAUNCHED.setdefault(self.test, set()).add(("192:" if self.mirror == "tile192" else "256:") + spec)
        pre = G.pre_act_ref(None, None, b64, None, self.st64, self.cs64, acc=self.acc)
        want = G.gemm_ref(None, None, b64, act, r64, rm, prefill, swiglu, None, self.st64, self.cs64, acc=self.acc)
        return o, want, pre

    def check(self, what, cfg, guard, out_dtype, **kw):
        o, want, _ = self.launch(cfg, guard, out_dtype, **kw)
        want = want.float() if out_dtype == F32 else G.to16(want, out_dtype, exact=True)
        o.check(want, f"{what} {_dt(self.dtype)} -> {_dt(out_dtype)} guard {guard} {sorted(k for k, v in kw.items() if v is not None and v is not False)}")

    def check_bounded(self, name, what, cfg, guard, out_dtype, act, swiglu=False, bias=True):
        o, ref, pre = self.launch(cfg, guard, out_dtype, act=act, swiglu=swiglu, bias=bias)
        if swiglu:
            g = pre.view(self.M, -1, 2, 16)
            b = G.bound(g[:, :, 0], G.ACT_SILU, up=g[:, :, 1]).reshape(self.M, -1)
        else:
            b = G.bound(pre, act)
        o.guards_kept(what)
        got = o.view.double()
        if out_dtype == F32:
            err = (got - ref).abs()
            r = torch.where(b > 0, err / b.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, G.INF), torch.zeros_like(err)))
            r = torch.where(torch.isnan(r), torch.full_like(r, G.INF), r)
            worst = float(r.max())
            WORST[name] = max(WORST.get(name, 0.0), worst)
            print(f"{name} {what} {_dt(self.dtype)} f32 out: {worst:.3g} of the bound")
            assert worst <= 1.0, f"{name} {what}: |err| / bound = {worst:.3g}"
        else:
            lo, hi = G.interval16(ref, b, out_dtype)
            out = ~((o.view >= lo) & (o.view <= hi))
            n = int(out.sum())
            print(f"{name} {what} {_dt(self.dtype)} guard {guard}: {n} of {out.numel()} outside [to16(ref - b), to16(ref + b)]")
            assert n == 0, f"{name} {what}: {n} of {out.numel()} 16-bit outputs outside the rounded interval"


@functools.lru_cache(maxsize=4)
def _small(M, N, K, seed):
    return G.small_ints(M, N, K, seed)


def _entry(name, table=None, **kw):
    M, N, K, cfg = G.reaches(name, table, **kw)
    return M, N, K, cfg, (table or G.BRANCHES)[name][4]


def _product_operands(kind, M, N, K):
    if kind == "ints":
        return G.ints(M, N, K, M + N + K)
    if kind == "round_bf16":
        return G.round_bf16(M, N, K, M + N + K + 1)
    return G.top_bf16(M, N, K, M + N + K + 2)[:2]


# ------------------------------------------------------------------------------------------------------ 1. exact products
@pytest.mark.parametrize("kind", ["ints", "round_bf16", "top_bf16"])
@pytest.mark.parametrize("branch", list(G.BRANCHES))
def test_exact_product(dev, branch, kind):
    """haff_gemm_{bf16,f16}{,_cfg,_ws} without an epilogue on every branch: f32 out == exact, 16-bit out == to16(exact). round_bf16:
    43 % of the results are bf16 ties (round-half-away and truncation fail); top_bf16: the largest finite bf16 stays finite, the
    tie above it stays finite in f32 and becomes inf in bf16. ints also in fp16. (An f32 output never meets a specialised
    instance's contract: on tile256_spec and tile192 it runs the generic one.)"""
    M, N, K, cfg, mirror = _entry(branch)
    a, w = _product_operands(kind, M, N, K)
    for dtype in (BF16, F16) if kind == "ints" else (BF16,):
        c = Case(dev, dtype, a, w, mirror, "test_exact_product")
        c.check(f"{branch} {kind}", cfg, 3, F32, bias=False)
        for guard in (64, 3):
            c.check(f"{branch} {kind}", cfg, guard, dtype, bias=False)


@pytest.mark.parametrize("name", list(G.PERSISTENT))
def test_exact_product_persistent_ring(dev, name):
    """the 8-wave tiles under gemm_stream_cap(8): several tiles per workgroup, the ring loop running across tile boundaries; plain,
    bias + residual and f32 out"""
    ops = _ops()
    M, N, K, cfg, mirror = _entry(name, G.PERSISTENT)
    assert G.tiles_per_workgroup(M, N, mirror, 8) >= 2
    ops.gemm_stream_cap(8)
    try:
        for kind in ("ints", "round_bf16"):
            a, w = _product_operands(kind, M, N, K)
            for dtype in (BF16, F16) if kind == "ints" else (BF16,):
                c = Case(dev, dtype, a, w, mirror, "test_exact_product_persistent_ring")
                c.check(f"{name} {kind}", cfg, 64, dtype, bias=False)
                c.check(f"{name} {kind}", cfg, 3, dtype, bias=False)
                c.check(f"{name} {kind}", cfg, 3, F32, bias=False)
        a, w = _small(M, N, K, 3)
        c = Case(dev, BF16, a, w, mirror, "test_exact_product_persistent_ring", bias=G.coded_bias(N))
        c.check(f"{name} coded", cfg, 64, BF16, resid=G.coded_resid(M, N))
    finally:
        ops.gemm_stream_cap(256)
    assert ops.gemm_stream_cap(0) == 256


@pytest.mark.parametrize("name", list(G.BIG))
def test_exact_product_large(dev, name):
    """1089 tiles of 128 x 128 (the two-K-tiles-in-flight loop switched off by the tile count) and outputs of exactly 64 MiB, which
    take the non-temporal stores: all three builders (ints also in fp16), the float64 reference on the device. nt_store_f32 is
    its fp32 output (64 MiB; the 16-bit output of that shape is half of it and another path); there round_bf16 has nothing to
    round and top_bf16 checks that the tie above the largest bf16 stays finite."""
    M, N, K, cfg, mirror = G.BIG[name]
    assert G.dispatch(M, N, K, cfg) == mirror
    f32 = name == "nt_store_f32"
    assert name == "tile128_many" or G.nt_store(M, N, f32)
    for kind in ("ints", "round_bf16", "top_bf16"):
        a, w = {"ints": lambda: G.ints(M, N, K, 5), "round_bf16": lambda: G.round_bf16(M, N, K, 6),
                "top_bf16": lambda: G.top_bf16(M, N, K, 7)[:2]}[kind]()
        for dtype in (BF16, F16) if kind == "ints" else (BF16,):
            c = Case(dev, dtype, a, w, mirror, "test_exact_product_large")
            c.check(f"{name} {kind}", cfg, 64, F32 if f32 else dtype, bias=False)
            del c


# ------------------------------------------------------------------------------------------------------ 2. exact epilogues
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt)
@pytest.mark.parametrize("branch", list(G.BRANCHES))
def test_exact_epilogue(dev, branch, dtype):
    """coded bias / residual / row map (terms that name their own index) and the rounds-ONCE case on every branch: bias; bias + ReLU;
    residual alone; bias + residual, also in place (out is resid); bias + residual + row map into M + 37 rows with 7 % dropped; f32
    out with an f32 residual; `once` (odd accumulators in the tie band, residual +-1) apart and in place. All ==.
    On tile256_spec the 64-guard launches meet HAFF_SPEC plain (test_exact_product), bias, res, bias_res (GF_RAGM forms, also on
    tile256_ragm); on tile192 HAFF_SPEC192 plain, bias, res, bias_res. bias_qgelu and the two swiglu instances are launched by
    test_activation_bounds, the LN instances by test_exact_folded_norm / test_activation_bounds / test_heads_scatter_exact, the
    statistics instances by test_rowstats_exact / test_rowstats32_exact, rope by test_qkv_rope_exact: every instance is reachable.
    Feature sets WITHOUT an instance fall to the generic one: ReLU / GELU / SiLU without LN, a row map without the head-major
    scatter, LN without bias or without column sums, LN + residual, any f32 output."""
    M, N, K, cfg, mirror = _entry(branch)
    a, w = _small(M, N, K, 7)
    c = Case(dev, dtype, a, w, mirror, "test_exact_epilogue", bias=G.coded_bias(N))
    rm, rows = G.coded_row_map(M, 9)
    resid, resid_rows = G.coded_resid(M, N), G.coded_resid(rows, N)
    assert float((c.acc + c.bias64).abs().max()) + 16 <= 256
    for guard in (64, 3):
        c.check(branch, cfg, guard, dtype)
        c.check(branch, cfg, guard, dtype, act=G.ACT_RELU)
        c.check(branch, cfg, guard, dtype, resid=resid)
        c.check(branch, cfg, guard, dtype, resid=resid, inplace=True)
        c.check(branch, cfg, guard, dtype, resid=resid_rows, row_map=rm, rows=rows)
    c.check(branch, cfg, 64, dtype, resid=resid, bias=False)
    c.check(branch, cfg, 3, F32, resid=resid)
    c.check(branch, cfg, 64, F32, resid=resid_rows, row_map=rm, rows=rows)
    a, w, r = G.once(M, N, K, 11, dtype)
    c = Case(dev, dtype, a, w, mirror, "test_exact_epilogue")
    c.check(f"{branch} once", cfg, 64, dtype, resid=r, bias=False)
    c.check(f"{branch} once", cfg, 3, dtype, resid=r, bias=False, inplace=True)


GATHER = {"skinny": G.AUTO["skinny"], "skinny_mt2_nt1": G.BRANCHES["skinny_mt2_nt1"], "skinny_mt4": G.BRANCHES["skinny_mt4"],
          "auto128": G.AUTO["auto128"], "auto256": G.AUTO["auto256"], "auto192": G.AUTO["auto192"]}


@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt)
@pytest.mark.parametrize("name", list(GATHER))
def test_exact_gather(dev, name, dtype):
    """haff_gemm_*_gather (no tile_cfg, no workspace: the tile is picked by shape): a gather map WITH REPEATS over M + 50 source rows,
    with bias, and with bias + residual + row map; =="""
    M, N, K, cfg, mirror = _entry(name, GATHER, a_map=True)
    a, w = _small(M + 50, N, K, 13)
    c = Case(dev, dtype, a, w, mirror, "test_exact_gather", bias=G.coded_bias(N), a_map=G.coded_a_map(M, M + 50, 14))
    assert c.M == M
    rm, rows = G.coded_row_map(M, 15)
    for guard in (64, 3):
        c.check(name, 0, guard, dtype)
        c.check(name, 0, guard, dtype, resid=G.coded_resid(rows, N), row_map=rm, rows=rows)
    c.check(name, 0, 3, F32)


# ---------------------------------------------------------------------------------------------------------- 3. folded norm
@pytest.mark.parametrize("rms", [False, True], ids=["layernorm", "rmsnorm"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt)
@pytest.mark.parametrize("name", ["skinny", "auto128", "auto256", "auto256_spec", "auto256_spec_ring"])
def test_exact_folded_norm(dev, name, dtype, rms):
    """haff_gemm_*_ln with integer means and power-of-two rstd (ln_exact): rstd * (acc - mean * colsum) + bias is exact in fp32 in
    any grouping, so f32 out == and 16-bit out == to16 of it; alone, + ReLU, + residual, + residual + row map. The tile is picked
    by shape: (300, 264, 256) is the generic 8-wave instance, (2816, 3072, 64) — 132 whole tiles, the least the auto rule gives the
    8-wave tile — meets HAFF_SPEC bias_ln_csum in the LayerNorm form (the RMS form, without column sums, has no instance), over
    one K-tile; (2816, 3072, 256) is the same launch over four K-tiles, the instance's ring loop."""
    M, N, K, cfg, mirror = _entry(name, G.AUTO, ln=True)
    d = G.ln_exact(M, N, K, 17, rms=rms)
    c = Case(dev, dtype, d["a"], d["w"], mirror, "test_exact_folded_norm", bias=d["bias"], ln_stats=d["ln_stats"], ln_colsum=d["ln_colsum"])
    rm, rows = G.coded_row_map(M, 19)
    for guard in (64, 3):
        c.check(name, 0, guard, dtype)
    c.check(name, 0, 3, F32)
    c.check(name, 0, 64, dtype, act=G.ACT_RELU)
    c.check(name, 0, 64, dtype, resid=G.coded_resid(M, N))
    c.check(name, 0, 3, dtype, resid=G.coded_resid(rows, N), row_map=rm, rows=rows)
    c.check(name, 0, 64, F32, resid=G.coded_resid(rows, N), row_map=rm, rows=rows)


# ----------------------------------------------------------------------------------------------------------- 4. activations
ACTS = {"gelu": G.ACT_GELU, "quick_gelu": G.ACT_QUICK_GELU, "silu": G.ACT_SILU}


@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt)
@pytest.mark.parametrize("branch", ["skinny_mt1", "skinny_mt2_nt1", "tile_splitk", "tile128", "tile256", "tile256_spec", "tile192"])
def test_activation_bounds(dev, branch, dtype):
    """GELU (polynomial erf), quick-GELU, SiLU and SwiGLU pairs (16-row interleaved gate | up, formed in the reduce kernel on
    tile_splitk) on pre-activations k / 4, |k| <= 48: f32 out within gemm_edge_ref.bound of the float64 result, 16-bit out inside the
    rounded interval. tile256_spec meets HAFF_SPEC bias_qgelu and swiglu, tile192 HAFF_SPEC192 swiglu."""
    M, N, K, cfg, mirror = _entry(branch)
    d = G.acts(M, N, K, 21)
    c = Case(dev, dtype, d["a"], d["w"], mirror, "test_activation_bounds", bias=d["bias"])
    for an, act in ACTS.items():
        c.check_bounded(f"{an} {branch}", branch, cfg, 3, F32, act)
        for guard in (64, 3):
            c.check_bounded(f"{an} {branch}", branch, cfg, guard, dtype, act)
    N2 = N // 32 * 32
    got = G.dispatch(M, N2, K, cfg, G.uses_workspace(M, cfg), swiglu=True)     # (SwiGLU pairs take two weight tiles per workgroup at least)
    assert got == mirror or (mirror.startswith("skinny") and got == mirror.rsplit("_nt", 1)[0] + "_nt2"), (got, mirror)
    d = G.acts(M, N2, K, 23)
    c = Case(dev, dtype, d["a"], d["w"], mirror, "test_activation_bounds", bias=d["bias"])
    c.check_bounded(f"swiglu {branch}", branch, cfg, 4, F32, 0, swiglu=True)     # (SwiGLU needs ldc % 4 == 0)
    c.check_bounded(f"swiglu {branch}", branch, cfg, 64, dtype, 0, swiglu=True)
    c.check_bounded(f"swiglu {branch}", branch, cfg, 4, dtype, 0, swiglu=True)
    c.check_bounded(f"swiglu {branch}", branch, cfg, 64, dtype, 0, swiglu=True, bias=False)   # (the specialised SwiGLU instances have no bias)


@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt)
@pytest.mark.parametrize("name", ["skinny", "auto128", "auto256_spec", "auto256_spec_ring"])
def test_activation_bounds_folded_norm(dev, name, dtype):
    """GELU behind a folded LayerNorm (the ViT-H lin1): exact pre-activations rstd * (acc - mean * colsum) + bias with |pre| <= 12;
    (2816, 3072, 64) meets HAFF_SPEC bias_ln_csum_gelu over one K-tile, (2816, 3072, 256) over four"""
    M, N, K, cfg, mirror = _entry(name, G.AUTO, ln=True)
    d = G.acts(M, N, K, 25, ln=True)
    c = Case(dev, dtype, d["a"], d["w"], mirror, "test_activation_bounds_folded_norm", bias=d["bias"], ln_stats=d["ln_stats"],
             ln_colsum=d["ln_colsum"])
    c.check_bounded(f"gelu+ln {name}", name, 0, 3, F32, G.ACT_GELU)
    for guard in (64, 3):
        c.check_bounded(f"gelu+ln {name}", name, 0, guard, dtype, G.ACT_GELU)


# ------------------------------------------------------------------------------------------------- 5. the fused producers
def _flat_guarded(n, dtype, dev):
    buf = torch.full((n + 128,), G.NAN, dtype=dtype, device=dev)
    return buf, buf[64:64 + n]


@pytest.mark.parametrize("fold", [False, True], ids=["plain", "ln"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt)
def test_heads_scatter_exact(dev, dtype, fold):
    """haff_gemm_*_heads at two whole 256-row tiles: column part * heads * d + h * d + c of row m lands at part * part_stride +
    h * head_stride + row_map[m] * d + c, dropped rows and unaddressed slots (the spare window, 64 guard elements on either side)
    keep their bits. With the folded LayerNorm this is HAFF_SPEC bias_ln_csum_map_hm."""
    ops = _ops()
    M, N, K, d, heads, ntok = 512, 512, 256, 64, 4, 49
    parts = N // (heads * d)
    assert ops.linear_heads_supported(M, N, K, d, heads, dtype)
    nwin = -(-M // ntok) + 1
    g = torch.Generator().manual_seed(27)
    slots = torch.randperm(nwin * ntok, generator=g)[:M]
    rm = torch.where(torch.rand((M,), generator=g) > 0.07, (slots // ntok) * (heads * ntok) + slots % ntok, torch.full((M,), -1)).to(torch.int32)
    if fold:
        c = G.ln_exact(M, N, K, 29)
    else:
        a, w = _small(M, N, K, 7)
        c = dict(a=a, w=w, bias=G.coded_bias(N), ln_stats=None, ln_colsum=None)
    y = G.pre_act_ref(c["a"].to(dev), c["w"].to(dev), c["bias"].to(dev), None, None if not fold else c["ln_stats"].to(dev),
                      None if not fold else c["ln_colsum"].to(dev))
    part_stride, head_stride = (nwin + 1) * heads * ntok * d, ntok * d
    n = parts * part_stride
    buf, out = _flat_guarded(n, dtype, dev)
    ops.linear_heads(_operand(c["a"], dtype, dev), _operand(c["w"], dtype, dev), _f32(c["bias"], dev), rm.to(dev), out, d, heads,
                     part_stride, head_stride, ln_stats=_f32(c["ln_stats"], dev), ln_colsum=_f32(c["ln_colsum"], dev))
    if fold:
        LAUNCHED.setdefault("test_heads_scatter_exact", set()).add("256:" + G.spec_instance(
            "tile256", M, N, d, False, bias=True, ln=True, csum=True, row_map=True, hm=True))
    want = torch.full((n + 128,), G.NAN, dtype=F64, device=dev)
    want[64:64 + n] = G.heads_ref(y, rm.to(dev), want[64:64 + n], d, heads, part_stride, head_stride)
    bad = _bad(buf, G.to16(want, dtype, exact=True))
    assert int(bad.sum()) == 0, f"{int(bad.sum())} of {bad.numel()} elements differ; first at {bad.nonzero()[:6].flatten().tolist()}"
    assert int(torch.isnan(buf).sum()) >= 128 + int((rm < 0).sum()) * N     # the guards and the dropped rows' slots stayed


@pytest.mark.parametrize("pos0", [0, 5])
@pytest.mark.parametrize("T", [256, 200], ids=["whole_tiles", "tile_spans_two_batches"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt)
def test_qkv_rope_exact(dev, dtype, T, pos0):
    """haff_gemm_*_qkv_rope (HAFF_SPEC rope) with cos / sin in {0, +-1, +-1/2} that change with every position and column
    (rope_exact): rotated q, the rotated k and the plain v at cache row (b, pos0 + t) are exact; cache rows outside the new
    positions and the guards of q keep their bits. T = 200: M = 400, a ragged last tile and a tile that spans both batch entries."""
    ops = _ops()
    import haff.ops as hops
    B, H, d, K = 2, 2, 128, 128
    M, hd = B * T, H * d
    Tmax = T + pos0 + 3
    assert ops.qkv_rope_supported(M, H, d, K, dtype, 1)
    a, w = G.ints(M, 3 * hd, K, 31)
    cs = G.rope_exact(Tmax)
    x, wp = _operand(a, dtype, dev), ops.rope_permute_rows(_operand(w, dtype, dev))
    kc = torch.full((B, Tmax, hd), G.NAN, dtype=dtype, device=dev)
    vc = torch.full_like(kc, G.NAN)
    q = Out(M, hd, dtype, dev, 64)
    csd = cs.float().contiguous().to(dev)
    lib = hops.load_library()
    rc = hops._fn(lib, "haff_gemm_bf16_qkv_rope", dtype)(x.data_ptr(), x.stride(0), wp.data_ptr(), wp.stride(0), q.view.data_ptr(), q.view.stride(0),
                                                        kc.data_ptr(), vc.data_ptr(), csd.data_ptr(), B, T, Tmax, pos0, H, d, K,
                                                        torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    LAUNCHED.setdefault("test_qkv_rope_exact", set()).add("256:" + G.spec_instance("tile256", M, 3 * hd, q.view.stride(0), False, rope=True))
    nan = torch.full((B, Tmax, hd), G.NAN, dtype=F64, device=dev)
    q64, k64, v64 = G.qkv_rope_ref(a.to(dev), w.to(dev), cs.to(dev), B, T, H, pos0, nan, nan)
    q.check(G.to16(q64, dtype, exact=True), "rotated q")
    for got, want, what in ((kc, k64, "k cache"), (vc, v64, "v cache")):
        bad = _bad(got, G.to16(want, dtype, exact=True))
        assert int(bad.sum()) == 0, f"{what}: {int(bad.sum())} of {bad.numel()} differ; first (b, row, col) {bad.nonzero()[:6].tolist()}"


def _ulps32(got, ref64):
    """|got - ref| in fp32 ulps of ref"""
    e = torch.floor(torch.log2(ref64.abs().clamp_min(2.0 ** -126)))
    return ((got.double() - ref64).abs() / torch.pow(2.0, e - 23)).max().item()


@pytest.mark.parametrize("gather", [False, True], ids=["plain", "gather"])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt)
def test_rowstats_exact(dev, dtype, gather):
    """haff_gemm_*_rowstats (HAFF_SPEC bias_res_stat) at (512, 512, 256): integer rows out = acc + bias + resid (|out| <= 256), apart
    and in place; the {sum, sum of squares} of every 64-column slot are exact (==), the finalised {mean, rstd} within 4 fp32 ulps."""
    ops = _ops()
    M, N, K, eps = 512, 512, 256, 1e-6
    assert ops.linear_rowstats_supported(M, N, K, dtype, 0)
    a, w = _small(M + 50 if gather else M, N, K, 13 if gather else 7)
    am = G.coded_a_map(M, M + 50, 33).to(dev) if gather else None
    bias, resid = G.coded_bias(N), G.coded_resid(M, N)
    x, wt = _operand(a, dtype, dev), _operand(w, dtype, dev)
    want = G.gemm_ref(a.to(dev), w.to(dev), bias.to(dev), 0, resid.to(dev), a_map=am)
    part_ref = G.rowstats_ref(want)
    for inplace in (False, True):
        o = Out(M, N, dtype, dev, 64)
        r = resid.to(dtype).to(dev)
        if inplace:
            o.view.copy_(r)
            r = o.view
        part = ops.rowstats_gemm(x, wt, _f32(bias, dev), r, o.view, a_map=am)
        LAUNCHED.setdefault("test_rowstats_exact", set()).add("256:" + G.spec_instance(
            "tile256", M, N, o.view.stride(0), False, bias=True, res=True, ldr=r.stride(0), stat=True))
        o.check(G.to16(want, dtype, exact=True), f"rowstats product inplace={inplace}")
        nbad = int((part.double() != part_ref).sum())
        assert nbad == 0, f"{nbad} of {part.numel()} partial sums differ"
    o = Out(M, N, dtype, dev, 64)
    _, st = ops.linear_rowstats(x, wt, _f32(bias, dev), resid.to(dtype).to(dev), eps, out=o.view, a_map=am)
    ref = G.stats_ref(want, eps)
    u = max(_ulps32(st[:, 0], ref[:, 0]), _ulps32(st[:, 1], ref[:, 1]))
    WORST[f"rowstats {_dt(dtype)} {{mean, rstd}} (bound: 4 ulps)"] = u / 4
    assert u <= 4.0, u


@pytest.mark.parametrize("gather", [False, True], ids=["plain", "gather"])
def test_rowstats32_exact(dev, gather):
    """haff_gemm_bf16_rowstats32 (HAFF_SPEC bias_res_stat_res32; bf16 only): the fp32 stream x32 += acc + bias in place is == exact,
    its bf16 copy == to16 of it (values up to 345: the odd ones above 256 need the rounding), slots ==, {mean, rstd} to 4 ulps."""
    ops = _ops()
    M, N, K, eps = 512, 512, 256, 1e-6
    a, w = G.small_ints(M + 50 if gather else M, N, K, 35, limit=80.0)
    am = G.coded_a_map(M, M + 50, 36).to(dev) if gather else None
    bias = G.coded_bias(N)
    x32_0 = G.coded_resid(M, N) * 16.0 + (torch.arange(N)[None, :] + torch.arange(M)[:, None]) % 2
    new, part_ref = G.rowstats32_ref(a.to(dev), w.to(dev), bias.to(dev), x32_0.to(dev), am)
    assert float(new.abs().max()) < 362 and float(new.abs().max()) > 256     # 64 squares below 2^17 each: the slot sums are exact
    x32 = Out(M, N, F32, dev, 64)
    x32.view.copy_(x32_0)
    o16 = Out(M, N, BF16, dev, 64)
    x, wt = _operand(a, BF16, dev), _operand(w, BF16, dev)
    part = ops.rowstats32_gemm(x, wt, _f32(bias, dev), x32.view, o16.view, a_map=am)
    LAUNCHED.setdefault("test_rowstats32_exact", set()).add("256:" + G.spec_instance(
        "tile256", M, N, o16.view.stride(0), False, bias=True, res32=True, stat=True))
    x32.check(new.float(), "fp32 stream")
    o16.check(G.to16(new, BF16, exact=True), "bf16 copy")
    assert int((part.double() != part_ref).sum()) == 0
    x32b = x32_0.float().to(dev).clone()
    st = ops.linear_rowstats32(x, wt, _f32(bias, dev), x32b, torch.empty((M, N), dtype=BF16, device=dev), eps, a_map=am)
    assert bool((x32b.double() == new).all())
    ref = G.stats_ref(new, eps)
    u = max(_ulps32(st[:, 0], ref[:, 0]), _ulps32(st[:, 1], ref[:, 1]))
    WORST["rowstats32 {mean, rstd} (bound: 4 ulps)"] = u / 4
    assert u <= 4.0, u


# ------------------------------------------------------------------------------------------------------------ 6. RMS carry
@pytest.mark.parametrize("N", [512, 1000])
@pytest.mark.parametrize("M", [1, 8, 16])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt)
def test_rms_carry_producer_exact(dev, dtype, M, N):
    """haff_gemm_*_rms producer: the residual product's output == to16(exact) (round_bf16 operands: results in the tie band, residual
    coded) and ssq_out[b][m] == the sum over workgroup b's 16 columns (8 in the last one at N = 1000) of the ROUNDED output squared —
    even integers up to 540, 16 squares below 2^19: exact. Rows m >= M of the 16 are UNTOUCHED (gemm_skinny_kernel returns at
    m >= p.M before the store): they keep the NaN they were filled with."""
    ops = _ops()
    H = 512
    a, w = G.round_bf16(M, N, H, 41) if dtype == BF16 else G.ints(M, N, H, 41)
    resid = G.coded_resid(M, N)
    o = Out(M, N, dtype, dev, 64)
    nb = -(-N // 16)
    parts = torch.full((nb + 2, 16), G.NAN, dtype=F32, device=dev)
    ops.linear_rms(_operand(a, dtype, dev), _operand(w, dtype, dev), resid=resid.to(dtype).to(dev), out=o.view, ssq_out=parts[1:nb + 1])
    want = G.to16(G.gemm_ref(a.to(dev), w.to(dev), resid=resid.to(dev)), dtype, exact=True)
    o.check(want, "rms producer output")
    exp = torch.full((nb + 2, 16), G.NAN, dtype=F64, device=dev)
    exp[1:nb + 1, :M] = G.rms_ssq_ref(want.double())
    assert float(exp[1:nb + 1, :M].max()) < 2.0 ** 24
    bad = _bad(parts, exp.float())
    assert int(bad.sum()) == 0, f"{int(bad.sum())} partials differ (rows m >= M and the guard rows must keep their NaN): {bad.nonzero()[:6].tolist()}"


@pytest.mark.parametrize("N2,swiglu", [(1000, False), (1024, True)])
@pytest.mark.parametrize("M", [1, 8])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt)
def test_rms_carry_consumer_bounded(dev, dtype, M, N2, swiglu):
    """haff_gemm_*_rms consumer (M <= 8) on hand-made partials: 32 producer workgroups hold 0.5 v_m and 1.5 v_m in turn, v_m = K (4^j -
    eps) / 32, j = m mod 3, eps = 2^-10; every sum of them is exact in fp32 in any order, sum / K + eps = 4^j and rstd = 2^-j up to one
    v_rsq_f32 rounding and one multiply: the f32 value lies within 2^-22 relative of 2^-j acc (exact). 16-bit output: inside the
    rounded interval. SwiGLU: silu'(g) <= 1.1, so the bound is b_silu(g) |u| + 2^-22 (1.1 |g| |u| + |silu(g) u|)."""
    ops = _ops()
    K, eps = 512, 2.0 ** -10
    a, w = G.small_ints(M, N2, K, 43, limit=128.0)
    w = w * 0.125
    j = (torch.arange(16) % 3).double()
    v = K * (torch.pow(4.0, j) - eps) / 32.0
    parts = v[None, :] * torch.where(torch.arange(32) % 2 == 0, 0.5, 1.5).double()[:, None]
    parts[:, M:] = 3.0                                             # rows m >= M: finite values nobody reads
    assert G.is16(parts, F32) and bool((G.rms_rstd_ref(parts[:, :M], K, eps) == torch.pow(2.0, -j[:M])).all())
    o = Out(M, N2 // 2 if swiglu else N2, dtype, dev, 64)
    ops.linear_rms(_operand(a, dtype, dev), _operand(w, dtype, dev), out=o.view, swiglu=swiglu, ssq_in=parts.float().to(dev), eps=eps)
    o.guards_kept("rms consumer")
    pre = G.rms_ref(a.to(dev), w.to(dev), parts.to(dev), eps)
    assert float(pre.abs().max()) <= 16.0
    rel = 2.0 ** -22
    if swiglu:
        g = pre.view(M, -1, 2, 16)
        g, u = g[:, :, 0], g[:, :, 1]
        ref = (G.act_ref(g, G.ACT_SILU) * u).reshape(M, -1)
        b = (G.bound(g, G.ACT_SILU, up=u) + rel * (1.1 * g.abs() * u.abs() + (G.act_ref(g, G.ACT_SILU) * u).abs())).reshape(M, -1)
    else:
        ref, b = pre, rel * pre.abs()
    lo, hi = G.interval16(ref, b, dtype)
    n = int((~((o.view >= lo) & (o.view <= hi))).sum())
    assert n == 0, f"{n} of {ref.numel()} outputs outside the rounded interval"


# -------------------------------------------------------------------------------------------------------------- 7. batched
@pytest.mark.parametrize("K", [72, 200], ids=["two_ktiles", "deep_k_with_tail"])
@pytest.mark.parametrize("shared_w", [False, True])
@pytest.mark.parametrize("dtype", [BF16, F16], ids=_dt)
def test_batched_exact(dev, dtype, shared_w, K):
    """haff_gemm_*_batched through autograd.bgemm: 2 x 3 batches of a ragged (130, 72, K) product with distinct outer and inner strides
    for A, W and C (every batch sits in a NaN slab of its own: a guard row above and below, guard columns, a spare inner slab), or W
    shared by the outer index (a zero stride); f32 and 16-bit out; == over the whole C allocation."""
    import haff  # noqa: F401
    from haff import autograd as ag
    M, N, Zo, Zi = 130, 72, 2, 3
    a, w = G.ints(Zo * Zi * M, (Zi if shared_w else Zo * Zi) * N, K, 51)
    A = torch.full((Zo, Zi + 1, M + 2, K + 8), G.NAN, dtype=dtype, device=dev)
    A[:, :Zi, 1:M + 1, :K] = a.view(Zo, Zi, M, K).to(dev)
    av = A[:, :Zi, 1:M + 1, :K]
    if shared_w:
        W = torch.full((Zi, N + 1, K + 8), G.NAN, dtype=dtype, device=dev)
        W[:, :N, :K] = w.view(Zi, N, K).to(dev)
        wv = W[None, :, :N, :K].expand(Zo, Zi, N, K)
        w64 = w.view(1, Zi, N, K).expand(Zo, Zi, N, K)
        assert wv.stride(0) == 0
    else:
        W = torch.full((Zo, Zi + 2, N + 1, K + 8), G.NAN, dtype=dtype, device=dev)
        W[:, :Zi, :N, :K] = w.view(Zo, Zi, N, K).to(dev)
        wv = W[:, :Zi, :N, :K]
        w64 = w.view(Zo, Zi, N, K)
    exact = torch.einsum("oimk,oink->oimn", a.view(Zo, Zi, M, K).to(dev), w64.to(dev))
    flat = G.batched_ref(a.reshape(-1), w64.contiguous().reshape(-1), torch.zeros(Zo * Zi * M * N, dtype=F64), K, Zi * M * K, M * K, K,
                         Zi * N * K, N * K, N, Zi * M * N, M * N, Zo, Zi, M, N, K)
    assert torch.equal(flat.view(Zo, Zi, M, N), exact.cpu())       # the strided restatement agrees with the einsum
    for out_dtype, guard in ((F32, 3), (dtype, 64), (dtype, 3)):
        C = torch.full((Zo, Zi + 1, M + 2, N + guard), G.NAN, dtype=out_dtype, device=dev)
        ag.bgemm(av, wv, out=C[:, :Zi, 1:M + 1, :N])
        exp = torch.full_like(C, G.NAN)
        exp[:, :Zi, 1:M + 1, :N] = exact.float() if out_dtype == F32 else G.to16(exact, out_dtype, exact=True)
        bad = _bad(C, exp)
        assert int(bad.sum()) == 0, f"{_dt(out_dtype)} guard {guard}: {int(bad.sum())} of {bad.numel()} differ; first {bad.nonzero()[:4].tolist()}"
