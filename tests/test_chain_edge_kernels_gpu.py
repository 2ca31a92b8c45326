"""The chained decode step (csrc/decode_chain.hip, through ops.decode_chain / ops.decode_chain_table) against tests/chain_ref.py, the
float64 restatement of haff_decode_chain_bf16 (checked on its own by tests/test_chain_ref_cpu.py), at the narrowest geometries the
entry point admits: hidden 256 / 2 heads / ffn 256 (a wave's whole K slice of o_proj and down_proj is one MFMA), 256 / 2 / 512 and
512 / 4 / 768, tmax 330, 1 to 8 rows with nk_rows on both sides of the 4-, 16-, 64- and 256-key edges, the empty cache (nk = 1) and
tmax itself; attention stages of 2, 4, 6, 8, 10, 12, 16, 20 and 32 workgroups, on both sides of the 8 counter shards.
test_decode_chain_gpu.py proves the CHAINING (chained == stage by stage) at 7B / 13B width; this module pins the ARITHMETIC:

  a. one layer with a known answer: x = e_m makes stage 0 hand on attn_edge_ref.rope_case's qkv_raw bit for bit, the rotated query
     picks ONE key (key 0, the new row, the last cached row, the first key of waves 1 to 3, keys 255 / 256 / 257 / 300), so att ==
     that V row; wo is a signed permutation and wd = 0, so the final x == r16(+-att[perm] + x), exactly;
  b. one layer of dense Gaussian operands, stage by stage, each stage against its restatement fed with what the DEVICE handed to
     that stage (a launch with wd = 0 shows x after o_proj), within the bounds of the existing edge suites: products and sums of
     squares train_edge_ref.bound / sum_bound, SwiGLU gemm_edge_ref.bound + interval16, attention attn_edge_ref.bound at U32;
  c. 1, 2 and 3 layers with weights and caches of their own: layer L of the (L + 1)-layer launch against the L-layer launch's final
     x and ssq_b, the layers below appending the same cache rows as the shorter launch;
  d. what the entry point refuses, with every buffer keeping its fill.

Every launch: x, qkv, att, g and the caches inside NaN-filled allocations with guard rows that must keep their bits, cache rows from
nk_rows[b] - 1 on NaN before the step, ssq_a / ssq_b NaN-filled (rows m >= M keep it); first the per-stage form, then the chained form
on fresh copies, ops.decode_chain_status after each (anything but True fails the test and bars the geometry for the session),
chained == per-stage bit for bit on x, qkv, att, g, ssq_a, ssq_b and both caches, a second chained run == the first. Every operand
stays inside the documented contract (1 <= nk_rows[b] <= tmax); nothing is meant to fault.

Measured on the MI355X (worst ratio to the bound over all cases; every equality held, no status word was set): qkv 0.999, x after
o_proj 0.999, x after down_proj 0.999 (the bound is half a bf16 ulp plus the fp32 evaluation's error: the stored values are
correctly rounded), g 0.996, att 0.5, the appended K row 0.5 ulps, ssq_a 0.111, ssq_b 0.111 (0.102 on the wd = 0 launches). In a.
`att == the chosen V row` held bit for bit on every case: the fall-back to attn_edge_ref.bound was not needed."""
import ctypes
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_edge_ref as A   # noqa: E402
import chain_ref as C   # noqa: E402

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
BAD_ARG, UNSUPPORTED = -1, -2
WORST = {}
_BARRED = set()      # geometries whose launch set the sticky timeout word: not launched again in this session
_EQUALITIES = ("same ", "==", "stages 0-3", "other ", "appended V", "inside", "cache rows")     # checks that answer 0 or inf


def _ops():
    import haff  # noqa: F401
    from haff import ops
    return ops


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for name in sorted(WORST):
        print(f"WORST {name}: {WORST[name]:.3g} of the bound")


def _settle(results, what):
    """print every figure, keep the worst per stage, then assert"""
    for name, v in results.items():
        stage = name.split(" ", 1)[1] if name[:1] == "L" and name[1:2].isdigit() else name
        if not any(w in stage for w in _EQUALITIES):
            WORST[stage] = max(WORST.get(stage, 0.0), v)
            print(f"{what} {name}: {v:.3g} of the bound")
    bad = {k: v for k, v in results.items() if not v <= 1.0}
    assert not bad, f"{what}: {bad}"


# ------------------------------------------------------------------------------------------------------------------ launches
class Guarded:
    """rows [R, C] as a view of a NaN-filled [R + 2, C] allocation: a guard row on either side"""

    def __init__(self, rows, dev, shape=None):
        R, Cc = rows.shape
        self.big = torch.full((R + 2, Cc), A.NAN, dtype=rows.dtype, device=dev)
        self.big[1:R + 1] = rows.to(dev)
        self.view = self.big[1:R + 1] if shape is None else self.big[1:R + 1].view(shape)
        assert self.view.is_contiguous() and self.view.data_ptr() % 16 == 0

    def get(self):
        big = self.big.cpu()
        want = torch.full((1,), A.NAN, dtype=big.dtype).view(torch.int16)
        assert bool((big[[0, -1]].view(torch.int16) == want).all()), "a guard row was written"
        return big[1:-1].view(self.view.shape)


def _nan(shape, dtype=BF16):
    return torch.full(shape, A.NAN, dtype=dtype)


class Step:
    """one fixture's operands on the device; launch(layers) runs the per-stage form, the chained form and the chained form again,
    each on fresh buffers, and returns the (bit-identical) result on the CPU"""

    def __init__(self, fx, dev):
        self.fx, self.dev = fx, dev
        self.hidden, self.heads, self.ffn = fx["geom"]
        self.nks, self.M = fx["nks"], len(fx["nks"])
        self.nk = torch.tensor(self.nks, dtype=torch.int32, device=dev)
        self.cs, self.stats0 = fx["cos_sin"].to(dev), fx["stats0"].to(dev)
        self.weights = {}

    def _w(self, t):
        """the device copy of a weight tensor (one per tensor of the fixture; a zeroed wd is a tensor of its own)"""
        if id(t) not in self.weights:
            self.weights[id(t)] = (t, t.to(self.dev))
        return self.weights[id(t)][1]

    def _once(self, layers, per_stage):
        ops, dev, M, H, F_ = _ops(), self.dev, self.M, self.hidden, self.ffn
        geom = self.fx["geom"]
        if geom in _BARRED:
            pytest.fail(f"geometry {geom}: an earlier launch ran out of patience (decode_chain_status); it is not launched again")
        n = len(layers)
        x, qkv, att, g = Guarded(self.fx["x"], dev), Guarded(_nan((M, 3 * H)), dev), Guarded(_nan((M, H)), dev), Guarded(_nan((M, F_)), dev)
        kcs = [Guarded(L[4].reshape(M * C.TMAX, H), dev, (M, C.TMAX, H)) for L in layers]
        vcs = [Guarded(L[5].reshape(M * C.TMAX, H), dev, (M, C.TMAX, H)) for L in layers]
        ssq_a, ssq_b = _nan((H // 16, 16), F32).to(dev), _nan((H // 16, 16), F32).to(dev)
        ws = torch.zeros((H // 16, 2, 16, 16), dtype=F32, device=dev)
        sync = torch.zeros((ops.decode_chain_sync_words(n, H),), dtype=torch.int32, device=dev)
        table = ops.decode_chain_table([tuple(self._w(t) for t in L[:4]) + (kcs[i].view, vcs[i].view) for i, L in enumerate(layers)])
        ops.decode_chain(table, n, x.view, qkv.view, att.view, g.view, ssq_a, ssq_b, ws, self.stats0, C.EPS, self.cs, self.nk, self.heads,
                         C.TMAX, C.SCALE, sync, per_stage_launches=per_stage)
        if ops.decode_chain_status(sync, n) is not True:
            _BARRED.add(geom)
            pytest.fail(f"geometry {geom}, {n} layers, nk_rows {self.nks}, per_stage {per_stage}: a bounded wait ran out (decode_chain_status)")
        got = dict(x=x.get(), qkv=qkv.get(), att=att.get(), g=g.get(), ssq_a=ssq_a.cpu(), ssq_b=ssq_b.cpu(), kc=[k.get() for k in kcs], vc=[v.get() for v in vcs])
        for name in ("ssq_a", "ssq_b"):     # rows m >= M of the partial sums are nobody's
            assert bool(torch.isnan(got[name][:, M:]).all()), f"{name}: a row past M was written"
        return got

    def launch(self, layers):
        what = f"geometry {self.fx['geom']} nk_rows {self.nks} {len(layers)} layers"
        stages = self._once(layers, True)
        chained = self._once(layers, False)
        bad = {k: v for k, v in C.same_launch(chained, stages).items() if v != 0.0}
        assert not bad, f"{what}: chained != per-stage: {sorted(bad)}"
        bad = {k: v for k, v in C.same_launch(self._once(layers, False), chained).items() if v != 0.0}
        assert not bad, f"{what}: a second chained run gave other bits: {sorted(bad)}"
        return chained


# ------------------------------------------------------------------------------------------------------------------ a, b, c
@pytest.mark.parametrize("case", C.onehot_cases(), ids=C.case_id)
def test_whole_layer_with_a_known_answer(dev, case):
    """a. qkv == qkv_raw, att == the chosen V row, the appended V row == v_new, the appended K row within one bf16 ulp of the float64
    rotation (the bar of test_decode_rope_appended_k_row), every other cache row keeps its bits, final x == r16(+-att[perm] + x0),
    ssq_a / ssq_b within sum_bound of the float64 group sums of that x, g within its interval on the device's x and ssq_a."""
    (hidden, heads, ffn), nks = case
    fx = C.onehot_fixture(hidden, heads, ffn, nks, 40 + C.onehot_cases().index(case))
    got = Step(fx, dev).launch(fx["layers"])
    _settle(C.check_onehot(fx, got), f"one-hot {C.case_id(case)}")


@pytest.mark.parametrize("case", C.dense_cases(), ids=C.case_id)
def test_stage_by_stage_on_dense_operands(dev, case):
    """b. two launches, wd = 0 and the real wd (stages 0 to 3 of the second bitwise those of the first); every stage's output
    against chain_ref's function for that stage on the device's own inputs to it."""
    (hidden, heads, ffn), nks = case
    fx = C.dense_fixture(hidden, heads, ffn, nks, 1, 11 + len(nks))
    _settle(C.check_prefix(fx, Step(fx, dev).launch), f"dense {C.case_id(case)}")


@pytest.mark.parametrize("case", C.prefix_cases(), ids=C.case_id)
def test_layer_handoffs_by_prefix_runs(dev, case):
    """c. n_layers = 1, 2, 3 on the same operands: the L-layer launch's qkv, att, g, final x, ssq_a and ssq_b are layer L's, checked
    as in b against the final x and ssq_b of the (L - 1)-layer launch (stats0 past layer 0, a ticket / counter offset or a cache
    pointer per layer would show); the layers below append the shorter launch's cache rows bit for bit."""
    (hidden, heads, ffn), nks = case
    fx = C.dense_fixture(hidden, heads, ffn, nks, 3, 23 + len(nks))
    _settle(C.check_prefix(fx, Step(fx, dev).launch), f"prefix {C.case_id(case)}")


# ------------------------------------------------------------------------------------------------------------------------ d
REFUSALS = (("M0", dict(M=0), BAD_ARG), ("M9", dict(M=9), BAD_ARG),
            ("hidden384", dict(hidden=384, heads=3), UNSUPPORTED), ("ffn384", dict(ffn=384), UNSUPPORTED),
            ("hidden_ne_128_heads", dict(heads=4), UNSUPPORTED), ("hidden_over_8192", dict(hidden=8448, heads=66), UNSUPPORTED),
            ("layers49", dict(n_layers=49), BAD_ARG), ("ws_misaligned", dict(ws_off=4), BAD_ARG), ("x_misaligned", dict(x_off=2), BAD_ARG),
            ("null_layer_pointer", dict(null="wo"), BAD_ARG))


@pytest.mark.parametrize("name,change,code", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_write_nothing(dev, name, change, code):
    """d. the error code, no launch: every buffer (the sync words included) keeps its fill; decode_chain_supported agrees on the
    geometry cases. The buffers are those of a valid (256, 2, 256) launch of 8 rows, so nothing could be written out of bounds."""
    ops = _ops()
    lib = ops.load_library()
    hidden, heads, ffn, M, n_layers = 256, 2, 256, 8, 1
    fill = lambda shape, dt, v: torch.full(shape, v, dtype=dt, device=dev)   # noqa: E731
    bufs = dict(x=fill((M, hidden), BF16, 3.0), qkv=fill((M, 3 * hidden), BF16, 3.0), att=fill((M, hidden), BF16, 3.0), g=fill((M, ffn), BF16, 3.0),
                ssq_a=fill((16, 16), F32, 3.0), ssq_b=fill((16, 16), F32, 3.0), ws=fill((16, 2, 16, 16), F32, 3.0),
                stats0=fill((M, 2), F32, 1.0), cos_sin=fill((C.TMAX, 128), F32, 1.0), nk=fill((M,), torch.int32, 1),
                sync=fill((ops.decode_chain_sync_words(1, hidden) + 64,), torch.int32, 3),
                wqkv=fill((3 * hidden, hidden), BF16, 3.0), wo=fill((hidden, hidden), BF16, 3.0), wgu=fill((2 * ffn, hidden), BF16, 3.0),
                wd=fill((hidden, ffn), BF16, 3.0), kc=fill((M, C.TMAX, hidden), BF16, 3.0), vc=fill((M, C.TMAX, hidden), BF16, 3.0))
    before = {k: v.clone() for k, v in bufs.items()}
    row = {k: bufs[n].data_ptr() for k, n in (("wqkv", "wqkv"), ("wo", "wo"), ("wgu", "wgu"), ("wd", "wd"), ("kcache", "kc"), ("vcache", "vc"))}
    if "null" in change:
        row[change["null"]] = None
    n_call = change.get("n_layers", n_layers)
    table = (ops.ChainLayer * n_call)(*[ops.ChainLayer(**row) for _ in range(n_call)])
    Mc, Hc, Fc, nh = change.get("M", M), change.get("hidden", hidden), change.get("ffn", ffn), change.get("heads", heads)
    rc = lib.haff_decode_chain_bf16(table, n_call, Mc, Hc, Fc, nh, bufs["x"].data_ptr() + change.get("x_off", 0), bufs["qkv"].data_ptr(),
                                    bufs["att"].data_ptr(), bufs["g"].data_ptr(), bufs["ssq_a"].data_ptr(), bufs["ssq_b"].data_ptr(),
                                    bufs["ws"].data_ptr() + change.get("ws_off", 0), bufs["stats0"].data_ptr(), C.EPS, bufs["cos_sin"].data_ptr(),
                                    bufs["nk"].data_ptr(), C.TMAX, C.SCALE, bufs["sync"].data_ptr(), 0, ops._stream())
    torch.cuda.synchronize()
    assert rc == code, f"{name}: returned {rc}, not {code}"
    for k, v in bufs.items():
        assert torch.equal(v, before[k]), f"{name}: {k} was written"
    if set(change) & {"M", "hidden", "ffn", "heads", "n_layers"}:
        assert not ops.decode_chain_supported(Mc, Hc, Fc, nh, n_call)
    assert ops.decode_chain_supported(M, hidden, ffn, heads, n_layers)


def test_supported_geometries_are_the_ones_tested(dev):
    ops = _ops()
    for hidden, heads, ffn in C.GEOMS:
        for M in (1, 8):
            for n in (1, 3, 48):
                assert ops.decode_chain_supported(M, hidden, ffn, heads, n)
    assert isinstance(ctypes.sizeof(ops.ChainLayer), int) and ctypes.sizeof(ops.ChainLayer) == 48
