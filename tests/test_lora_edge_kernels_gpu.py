"""The adapter kernels of csrc/lora.hip that were reached only through the autograd nodes — haff_lora_qkv_rope_fwd, haff_lora_qkv3_rope_fwd,
haff_lora_qkv_rope_bwd, haff_lora_dx, haff_lora_dx2, haff_lora_dx3 — and haff_lora_tn at the small edges of its row-block geometry,
each called through its C entry point in both 16-bit types and compared with the float64 restatements of tests/lora_edge_ref.py
(checked on their own by tests/test_lora_edge_ref_cpu.py).

Exact family (small integers, masks in {0, 1, 2}, power-of-two scale, quarter-turn RoPE tables: every partial sum and result an
integer <= 256) is compared with ==, on the WHOLE allocation: every output and in/out buffer is a view of a longer one prefilled
with the sentinel, rows past M and the columns between the width and the leading dimension included, and the expectation holds the
sentinel there. With accumulate = 0 the destination holds NaN and has to come out finite and equal. Inputs are compared with their
clones after every call. Gauss family (the trainer's magnitudes) is held to K times the fp32 evaluation's worst error, FLOOR_ULPS
fp32 ulps of the sum of absolute terms and half a storage ulp. The three grid-capped kernels run past their caps once per entry point (258 row
tiles against 4 x 64; 4 194 456 threads against 16384 x 256), the reference evaluated on the device in float64 row slabs. Every
documented refusal has to return its code and leave every output untouched. Each comparison prints its ratio to the bound; the
module prints the worst per kernel and output at the end.

Measured on the MI355X (51 tests, 5.7 to 6.1 s for the file; the slowest, the three-adapter forward past the cap, 0.55 s): every exact
case has 0 entries that differ (576 forward, 288 adjoint, 1536 dx, 2560 tn, the probes, the seven past-the-cap cases, each under
2 GiB of device memory). Worst |error| / bound of the Gauss family: 0.9991 to 0.9995 for every 16-bit output (half a storage ulp is
nearly the whole of that bound), tn with f32 out 0.109. No defect and no missing refusal was found; csrc/lora.hip is unchanged."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_edge_ref as R   # noqa: E402
import lora_edge_ref as L   # noqa: E402

pytestmark = pytest.mark.gpu

BAD_ARG, UNSUPPORTED = -1, -2
F32, F64, BF16, F16 = R.F32, R.F64, R.BF16, R.F16
NAN, SENT = R.NAN, R.SENT
_id = lambda v: L.IDS.get(v, None)   # noqa: E731
WORST = {}
EXTRA = 3                 # sentinel rows after row M of every output


def _lib():
    import haff  # noqa: F401
    from haff.lib import load_library
    return load_library()


def _s():
    return torch.cuda.current_stream().cuda_stream


def _fn(lib, stem, dtype):
    return getattr(lib, stem + ("_f16" if dtype == F16 else ""))


def _check(name, got, ref, bnd, what=""):
    r = R.ratio(got, ref, bnd)
    WORST[name] = max(WORST.get(name, 0.0), r)
    print(f"{name} {what}: ratio to bound {r:.3g}")
    assert r <= 1.0, f"{name} {what}: |err| / bound = {r:.3g}"


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for name in sorted(WORST):
        print(f"WORST {name}: {WORST[name]:.4f}")


def _bits(t):
    return t.view(torch.int32 if t.dtype == F32 else torch.int16)


class Out:
    """A [rows + EXTRA][ld] buffer for a kernel to write its [rows][width] share of, inside a longer allocation, all of it prefilled
    with the sentinel; `body` (a tensor, or a number such as NaN) prefills the share."""

    def __init__(self, rows, width, ld, dtype, dev, body=None, edge=64):
        self.rows, self.width, self.ld, self.edge = rows + EXTRA, width, ld, edge
        self.flat = torch.full((2 * edge + self.rows * ld,), SENT, dtype=dtype, device=dev)
        self.t = self.flat[edge:edge + self.rows * ld].view(self.rows, ld)
        if body is not None:
            self.t[:rows, :width] = body
        self.before = self.flat.clone()

    @property
    def ptr(self):
        return self.t.data_ptr()

    def _edges(self):
        return bool((self.flat[:self.edge] == SENT).all()) and bool((self.flat[-self.edge:] == SENT).all())

    def equals(self, expected):
        """the whole buffer, the sentinel regions included, against `expected` [rows + EXTRA][ld]"""
        assert self._edges(), "written outside the allocation's view"
        return torch.equal(self.t, expected.to(self.t.device))

    def body(self, M):
        """the kernel's share on the CPU, after checking that everything around it still holds the sentinel"""
        assert self._edges(), "written outside the allocation's view"
        t = self.t.cpu()
        assert bool((t[M:] == SENT).all()) and bool((t[:, self.width:] == SENT).all()), "rows past M or the columns past the width were written"
        return t[:M, :self.width]

    def untouched(self):
        return torch.equal(_bits(self.flat), _bits(self.before))


class In:
    """An operand on the device as the [r][c] view of a [r + more_rows][ld] tensor of `fill`, with a clone to compare with afterwards"""

    def __init__(self, x, ld, dev, fill, more_rows=0):
        self.full = L.pad2d(x, x.shape[0] + more_rows, ld, fill).to(dev)
        self.before = self.full.clone()
        self.ld = ld

    @property
    def ptr(self):
        return self.full.data_ptr()

    def unchanged(self):
        return torch.equal(_bits(self.full), _bits(self.before))


# ---------------------------------------------------------------------------------------------------------------- runners
def _run_fwd(lib, dev, inp, cs, T, H, na, dtype, layout):
    """-> the three Outs. qkv ends at its row M (no row after the last to read), NaN in its padding columns; t^T pads 3.0"""
    M = inp["qkv"].shape[0]
    d = L.lds(layout, M, H)
    ins = [In(inp["qkv"], d["w3"], dev, NAN), In(inp["tT"], d["ldt"], dev, 3.0)]
    ins += [In(inp[n], 8, dev, 0.0) for n in ("Bq", "Bv", "Bk")[:na]] + [In(cs, L.HD, dev, NAN)]
    outs = [Out(M, H, d["w"], dtype, dev) for _ in range(3)]
    B = [i.ptr for i in ins[2:2 + na]]
    fn = _fn(lib, "haff_lora_qkv3_rope_fwd" if na == 3 else "haff_lora_qkv_rope_fwd", dtype)
    rc = fn(ins[0].ptr, d["w3"], ins[1].ptr, d["ldt"], *B, 8, ins[-1].ptr, outs[0].ptr, outs[1].ptr, outs[2].ptr, d["w"], M, H, L.HD, T,
            inp["scale"], _s())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert all(i.unchanged() for i in ins), "an input was modified"
    return outs


def _run_bwd(lib, dev, grads, cs, T, H, dtype, layout):
    M = grads[0].shape[0]
    d = L.lds(layout, M, H)
    ins = [In(g, d["w"], dev, NAN) for g in grads] + [In(cs, L.HD, dev, NAN)]
    out = Out(M, 3 * H, d["w3"], dtype, dev)
    rc = _fn(lib, "haff_lora_qkv_rope_bwd", dtype)(ins[0].ptr, ins[1].ptr, ins[2].ptr, d["w"], ins[3].ptr, out.ptr, d["w3"], M, H, L.HD, T, _s())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert all(i.unchanged() for i in ins), "an input was modified"
    return out


DX_ARRANGEMENTS = (("haff_lora_dx", 2, 0), ("haff_lora_dx", 2, 1), ("haff_lora_dx2", 2, 2), ("haff_lora_dx3", 3, 0), ("haff_lora_dx3", 3, 1),
                   ("haff_lora_dx3", 3, 3))     # (entry point, adapters, masks): every arrangement the entry points accept


def _run_dx(lib, dev, inp, stem, na, nm, accumulate, dtype, layout):
    """-> the destination Out: prefilled with dx0 (accumulate = 1) or NaN (accumulate = 0)"""
    M, Kd = inp["dx0"].shape
    d = L.lds(layout, M, Kd)
    ins = [In(inp["dtT"], d["ldt"], dev, 3.0), In(inp["A"], d["lda"], dev, NAN)] + [In(k, d["w"], dev, NAN) for k in inp["keeps"][:nm]]
    keeps = [i.ptr for i in ins[2:]]
    out = Out(M, Kd, d["w"], dtype, dev, body=inp["dx0"].to(dev) if accumulate else NAN)
    if stem == "haff_lora_dx":
        masks = [keeps[0] if nm else None]
    elif stem == "haff_lora_dx2":
        masks = keeps
    else:
        masks = (keeps + [None] * 3)[:3]
    rc = _fn(lib, stem, dtype)(ins[0].ptr, d["ldt"], ins[1].ptr, d["lda"], *masks, d["w"], out.ptr, d["w"], int(accumulate), M, Kd, inp["scale"], _s())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert all(i.unchanged() for i in ins), "an input was modified"
    return out


def _fwd_args(inp, cs, T, H):
    return (inp["qkv"], inp["tT"], inp["Bq"], inp["Bv"], inp["Bk"], cs, T, H, inp["scale"])


def _dx_args(inp, nm, accumulate, na):
    return (inp["dtT"], inp["A"], inp["keeps"][:nm], inp["dx0"] if accumulate else None, inp["scale"], na)


# -------------------------------------------------------------------------------------------------------- the exact family
@pytest.mark.parametrize("dtype", L.HALF, ids=_id)
@pytest.mark.parametrize("na", (2, 3))
def test_forward_exact(dev, na, dtype):
    """q, k, v == the restatement at every M x H x T x layout of the lists, the whole sentinel-filled buffers compared"""
    lib, n = _lib(), 0
    for M in L.ROWS:
        for H in L.WIDTHS:
            inp = L.fwd_inputs("exact", M, H, na, M + H + na, dtype)
            for T in L.t_values(M):
                cs = L.quarter_turns(T)
                ref = L.qkv_rope_fwd(*_fwd_args(inp, cs, T, H))
                for layout in L.LAYOUTS:
                    outs = _run_fwd(lib, dev, inp, cs, T, H, na, dtype, layout)
                    for name, o, r in zip("qkv", outs, ref):
                        assert o.equals(L.embed(r, o.rows, o.ld, dtype)), f"{name} M {M} H {H} T {T} {layout} na {na}"
                    n += 1
    print(f"forward exact na {na} {L.IDS[dtype]}: {n} cases, 0 entries differ")


@pytest.mark.parametrize("dtype", L.HALF, ids=_id)
def test_forward_rank_probes_and_k_only(dev, dtype):
    """t one-hot in rank (row mod 8 na) against B with a distinct integer per (column mod 128, rank): column c of head h takes exactly
    row c of B, rank j exactly row 8a + j of t^T, its partner at c +- 64. k only: the q and v rank rows are zero, Bq and Bv are not."""
    lib = _lib()
    for na in (2, 3):
        for M, H, T, layout in ((100, 384, 7, "padded"), (65, 128, 65, "odd"), (17, 384, 1, "tight")):
            for kind in ("probe", "k_only") if na == 3 else ("probe",):
                inp = L.fwd_inputs("probe" if kind == "probe" else "exact", M, H, na, M + na, dtype, k_only=kind == "k_only")
                cs = L.quarter_turns(T)
                ref = L.qkv_rope_fwd(*_fwd_args(inp, cs, T, H))
                if kind == "k_only":
                    assert torch.equal(ref[2], inp["qkv"].double()[:, 2 * H:])
                for name, o, r in zip("qkv", _run_fwd(lib, dev, inp, cs, T, H, na, dtype, layout), ref):
                    assert o.equals(L.embed(r, o.rows, o.ld, dtype)), f"{kind} {name} M {M} H {H} T {T} {layout} na {na}"


@pytest.mark.parametrize("dtype", L.HALF, ids=_id)
def test_adjoint_exact(dev, dtype):
    """dqkv == [rope^T dq | rope^T dk | dv] at every M x H x T x layout; the dv third is the input's bits"""
    lib, n = _lib(), 0
    for M in L.ROWS:
        for H in L.WIDTHS:
            grads = L.bwd_inputs("exact", M, H, M + H, dtype)
            for T in L.t_values(M):
                cs = L.quarter_turns(T)
                ref = L.qkv_rope_bwd(*grads, cs, T, H)
                for layout in L.LAYOUTS:
                    o = _run_bwd(lib, dev, grads, cs, T, H, dtype, layout)
                    assert o.equals(L.embed(ref, o.rows, o.ld, dtype)), f"M {M} H {H} T {T} {layout}"
                    n += 1
    print(f"adjoint exact {L.IDS[dtype]}: {n} cases, 0 entries differ")


@pytest.mark.parametrize("dtype", L.HALF, ids=_id)
@pytest.mark.parametrize("stem,na,nm", DX_ARRANGEMENTS, ids=lambda v: str(v).replace("haff_lora_", ""))
def test_dx_exact(dev, stem, na, nm, dtype):
    """dx == the restatement with accumulate 0 (destination prefilled with NaN) and 1 (with dx0), at every M x K x layout, for every
    mask arrangement; the probe inputs (dt one-hot in rank row mod 8 na, a distinct integer per (column mod 128, rank) in A) as well"""
    lib, n = _lib(), 0
    for M in L.ROWS:
        for Kd in L.WIDTHS:
            for family in ("exact", "probe"):
                inp = L.dx_inputs(family, M, Kd, na, nm, M + Kd + na + nm, dtype)
                for acc in (0, 1):
                    ref = L.dx(*_dx_args(inp, nm, acc, na))
                    for layout in L.LAYOUTS if family == "exact" else ("padded",):
                        o = _run_dx(lib, dev, inp, stem, na, nm, acc, dtype, layout)
                        assert o.equals(L.embed(ref, o.rows, o.ld, dtype)), f"{stem} {family} M {M} K {Kd} accumulate {acc} {layout}"
                        n += 1
    print(f"{stem} na {na} masks {nm} {L.IDS[dtype]}: {n} cases, 0 entries differ")


def _run_tn(lib, dev, sT_in, big_in, ws, M, N, Rr, j_valid, transposed, out_f32, dtype, scale):
    """one launch on the given operands and workspace -> the Out"""
    odt = F32 if out_f32 else dtype
    out = Out(N, j_valid, j_valid + 2, odt, dev) if transposed else Out(j_valid, N, N + 8, odt, dev)
    rc = _fn(lib, "haff_lora_tn", dtype)(sT_in.ptr, sT_in.ld, Rr, big_in.ptr, big_in.ld, M, N, ws.ptr, ws.width, out.ptr, out.ld, out_f32,
                                         transposed, j_valid, scale, _s())
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("dtype", L.HALF, ids=_id)
@pytest.mark.parametrize("Rr", L.TN_R)
def test_tn_exact(dev, Rr, dtype):
    """haff_lora_tn == scale sT[:, :M] big on integer operands at every M x N of the lists, both layouts, j_valid in {1, R - 3, R},
    f32 and 16-bit out, lds = roundup(M, 16) and 8 more (pads 3.0), ldb = N + 2 (columns past N 5.0), on a workspace of exactly
    haff_lora_tn_workspace_elems values; a second launch on the same workspace gives the same bits"""
    lib, n = _lib(), 0
    for M in L.TN_M:
        for N in L.TN_N:
            inp = L.tn_inputs("exact", M, N, Rr, M + N + Rr, dtype)
            n_ws = lib.haff_lora_tn_workspace_elems(M, Rr, N)
            assert n_ws == L.tn_geometry(M)[1] * Rr * N
            big_in = In(inp["big"], N + 2, dev, 5.0)
            sTs = [In(inp["sT"], -(-M // 16) * 16 + more, dev, 3.0) for more in (0, 8)]
            ref = L.lora_tn(inp["sT"], inp["big"], M, inp["scale"], Rr, 0)
            for transposed in (0, 1):
                for j_valid in (1, Rr - 3, Rr):
                    for out_f32 in (1, 0):
                        odt = F32 if out_f32 else dtype
                        want = ref[:j_valid].T if transposed else ref[:j_valid]
                        for sT_in in sTs if j_valid == Rr else sTs[:1]:
                            ws = Out(1, n_ws, n_ws, F32, dev)
                            outs = [_run_tn(lib, dev, sT_in, big_in, ws, M, N, Rr, j_valid, transposed, out_f32, dtype, inp["scale"]) for _ in range(2)]
                            torch.cuda.synchronize()
                            what = f"M {M} N {N} R {Rr} transposed {transposed} j_valid {j_valid} out_f32 {out_f32} lds {sT_in.ld}"
                            assert outs[0].equals(L.embed(want, outs[0].rows, outs[0].ld, odt)), what
                            assert torch.equal(_bits(outs[0].flat), _bits(outs[1].flat)), "a second launch gave other bits: " + what
                            ws.body(1)       # nothing written around the workspace
                            n += 1
            assert big_in.unchanged() and all(s.unchanged() for s in sTs)
    print(f"tn exact R {Rr} {L.IDS[dtype]}: {n} cases, 0 entries differ")


# -------------------------------------------------------------------------------------------------------- the Gauss family
def _gauss_shapes():
    """every M at three heads / K = 384, T = 7, the padded layout; the other width, the other T and the other layouts at M = 100 and 17"""
    s = [(M, 384, 7, "padded") for M in L.ROWS]
    return s + [(100, 128, 100, "tight"), (100, 384, 1, "odd"), (17, 128, 17, "odd"), (17, 384, 7, "tight")]


@pytest.mark.parametrize("dtype", L.HALF, ids=_id)
def test_forward_and_adjoint_gauss(dev, dtype):
    lib = _lib()
    for M, H, T, layout in _gauss_shapes():
        cs = L.angle_table(T)
        for na in (2, 3):
            inp = L.fwd_inputs("gauss", M, H, na, M + H + na, dtype)
            exp = L.expect(L.qkv_rope_fwd, _fwd_args(inp, cs, T, H), (dtype,) * 3)
            for name, o, (ref, bnd) in zip("qkv", _run_fwd(lib, dev, inp, cs, T, H, na, dtype, layout), exp):
                _check(f"forward na {na} {name}", o.body(M), ref, bnd, f"M {M} H {H} T {T} {layout} {L.IDS[dtype]}")
        grads = L.bwd_inputs("gauss", M, H, M + H, dtype)
        (ref, bnd), = L.expect(L.qkv_rope_bwd, (*grads, cs, T, H), dtype)
        got = _run_bwd(lib, dev, grads, cs, T, H, dtype, layout).body(M)
        _check("adjoint dqkv", got, ref, bnd, f"M {M} H {H} T {T} {layout} {L.IDS[dtype]}")
        assert torch.equal(_bits(got[:, 2 * H:].contiguous()), _bits(grads[2].contiguous())), "dv is not copied bit for bit"


@pytest.mark.parametrize("dtype", L.HALF, ids=_id)
def test_dx_gauss(dev, dtype):
    lib = _lib()
    for M, Kd, _, layout in _gauss_shapes():
        for stem, na, nm in DX_ARRANGEMENTS:
            inp = L.dx_inputs("gauss", M, Kd, na, nm, M + Kd + na + nm, dtype)
            for acc in (0, 1):
                (ref, bnd), = L.expect(L.dx, _dx_args(inp, nm, acc, na), dtype)
                got = _run_dx(lib, dev, inp, stem, na, nm, acc, dtype, layout).body(M)
                _check(f"{stem[10:]} masks {nm} accumulate {acc}", got, ref, bnd, f"M {M} K {Kd} {layout} {L.IDS[dtype]}")


@pytest.mark.parametrize("dtype", L.HALF, ids=_id)
def test_tn_gauss(dev, dtype):
    lib = _lib()
    for M in L.TN_M:
        for N, Rr in ((130, 16), (126, 8), (2, 16)):
            inp = L.tn_inputs("gauss", M, N, Rr, M + N, dtype)
            n_ws = lib.haff_lora_tn_workspace_elems(M, Rr, N)
            sT_in, big_in = In(inp["sT"], -(-M // 16) * 16, dev, 3.0), In(inp["big"], N + 2, dev, 5.0)
            for transposed, j_valid, out_f32 in ((0, Rr, 1), (1, Rr - 3, 0), (0, Rr, 0), (1, 1, 1)):
                odt = F32 if out_f32 else dtype
                (ref, bnd), = L.expect(L.lora_tn, (inp["sT"], inp["big"], M, inp["scale"], j_valid, transposed), odt)
                ws = Out(1, n_ws, n_ws, F32, dev)
                out = _run_tn(lib, dev, sT_in, big_in, ws, M, N, Rr, j_valid, transposed, out_f32, dtype, inp["scale"])
                torch.cuda.synchronize()
                _check("tn f32" if out_f32 else "tn 16-bit", out.body(N if transposed else j_valid), ref, bnd,
                       f"M {M} N {N} R {Rr} transposed {transposed} j_valid {j_valid} {L.IDS[dtype]}")


# ---------------------------------------------------------------------------------------------------------- past the caps
def _mem_mark():
    """-> what is allocated on the device before the case starts (other modules' tensors included)"""
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    return torch.cuda.memory_allocated()


def _peak_ok(what, base):
    peak = torch.cuda.max_memory_allocated() - base
    print(f"{what}: peak device memory of the case {peak / 2 ** 30:.2f} GiB")
    assert peak < 4 * 10 ** 9, peak


def _slabs(M):
    return [(r0, min(r0 + L.SLAB, M)) for r0 in range(0, M, L.SLAB)]


@pytest.mark.parametrize("na,dtype", ((3, BF16), (2, F16)), ids=("qkv3-bf16", "qkv-f16"))
def test_forward_past_the_cap(dev, na, dtype):
    """H = 4096 (cap 64 workgroups in y), M = 4115: 258 row tiles, tiles 256 and 257 on the second trip of `rt += gridDim.y * 4`,
    the last with 3 rows; three adapters in bf16, two in f16. Exact family, ==, the reference in float64 on the device."""
    lib, M, H, T = _lib(), L.BIG_FWD["M"], L.BIG_FWD["H"], 7
    assert -(-M // 16) > 4 * -(-L.FWD_CAP // (H // L.HD))
    base = _mem_mark()
    inp = L.fwd_inputs("exact", M, H, na, 11, dtype, device=dev)
    cs = L.quarter_turns(T, device=dev)
    before = {k: v.clone() for k, v in inp.items() if torch.is_tensor(v)}
    outs = [Out(M, H, H + 8, dtype, dev) for _ in range(3)]
    B = [inp[n].data_ptr() for n in ("Bq", "Bv", "Bk")[:na]]
    fn = _fn(lib, "haff_lora_qkv3_rope_fwd" if na == 3 else "haff_lora_qkv_rope_fwd", dtype)
    rc = fn(inp["qkv"].data_ptr(), 3 * H, inp["tT"].data_ptr(), M, *B, 8, cs.data_ptr(), outs[0].ptr, outs[1].ptr, outs[2].ptr, H + 8, M, H, L.HD, T,
            inp["scale"], _s())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert all(torch.equal(inp[k], v) for k, v in before.items()), "an input was modified"
    del before
    exp = [torch.full((o.rows, o.ld), SENT, dtype=dtype, device=dev) for o in outs]
    for r0, r1 in _slabs(M):
        ref = L.qkv_rope_fwd(inp["qkv"][r0:r1], inp["tT"][:, r0:r1], inp["Bq"], inp["Bv"], inp["Bk"], cs, T, H, inp["scale"], row0=r0)
        for e, r in zip(exp, ref):
            assert float(r.abs().max()) <= L.EXACT_MAX
            e[r0:r1, :H] = r.to(dtype)
        del ref
    for name, o, e in zip("qkv", outs, exp):
        bad = int((o.t != e).sum())
        print(f"forward past the cap {name}: {bad} entries differ")
        assert o.equals(e), f"{name}: {bad} entries differ, first rows {(o.t != e).any(1).nonzero()[:4].flatten().tolist()}"
    _peak_ok("forward past the cap", base)


@pytest.mark.parametrize("stem,na,nm,dtype", (("haff_lora_dx3", 3, 3, F16), ("haff_lora_dx2", 2, 2, BF16), ("haff_lora_dx", 2, 1, BF16)),
                         ids=("dx3-f16", "dx2-bf16", "dx-bf16"))
def test_dx_past_the_cap(dev, stem, na, nm, dtype):
    """accumulate = 1, K = 4096 (cap 64), M = 4115: the same second trip in lora_dx_kernel, with three masks in f16, two and one in bf16"""
    lib, M, Kd = _lib(), L.BIG_DX["M"], L.BIG_DX["Kd"]
    assert -(-M // 16) > 4 * -(-L.FWD_CAP // (Kd // 128))
    base = _mem_mark()
    inp = L.dx_inputs("exact", M, Kd, na, nm, 13, dtype, device=dev)
    keeps = inp["keeps"]
    before = [t.clone() for t in (inp["dtT"], inp["A"], *keeps)]
    out = Out(M, Kd, Kd + 8, dtype, dev, body=inp["dx0"])
    rc = _fn(lib, stem, dtype)(inp["dtT"].data_ptr(), M, inp["A"].data_ptr(), Kd, *[k.data_ptr() for k in keeps], Kd, out.ptr, Kd + 8, 1, M, Kd,
                               inp["scale"], _s())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (inp["dtT"], inp["A"], *keeps))), "an input was modified"
    del before
    exp = torch.full((out.rows, out.ld), SENT, dtype=dtype, device=dev)
    for r0, r1 in _slabs(M):
        ref = L.dx(inp["dtT"][:, r0:r1], inp["A"], tuple(k[r0:r1] for k in keeps), inp["dx0"][r0:r1], inp["scale"], na)
        assert float(ref.abs().max()) <= L.EXACT_MAX
        exp[r0:r1, :Kd] = ref.to(dtype)
        del ref
    bad = int((out.t != exp).sum())
    print(f"{stem} past the cap: {bad} entries differ")
    assert out.equals(exp), f"{bad} entries differ, first rows {(out.t != exp).any(1).nonzero()[:4].flatten().tolist()}"
    _peak_ok(f"{stem} past the cap", base)


@pytest.mark.parametrize("dtype", L.HALF, ids=_id)
def test_adjoint_past_the_cap(dev, dtype):
    """H = 128, M = 524307: M * nh * 8 = 4 194 456 threads of work against 16384 blocks of 256: the last 152 (19 rows) are the
    second trip of `i += gridDim.x * blockDim.x`"""
    lib, M, H, T = _lib(), L.BIG_BWD["M"], L.BIG_BWD["H"], 7
    assert M * (H // L.HD) * 8 > L.BWD_CAP
    base = _mem_mark()
    grads = L.bwd_inputs("exact", M, H, 17, dtype, device=dev)
    cs = L.quarter_turns(T, device=dev)
    before = [g.clone() for g in grads]
    out = Out(M, 3 * H, 3 * H, dtype, dev)
    rc = _fn(lib, "haff_lora_qkv_rope_bwd", dtype)(grads[0].data_ptr(), grads[1].data_ptr(), grads[2].data_ptr(), H, cs.data_ptr(), out.ptr, 3 * H, M, H, L.HD, T, _s())
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, grads)), "an input was modified"
    del before
    assert bool((out.t[M:] == SENT).all()) and out._edges()
    for r0, r1 in _slabs(M):
        ref = L.qkv_rope_bwd(grads[0][r0:r1], grads[1][r0:r1], grads[2][r0:r1], cs, T, H, row0=r0).to(dtype)
        bad = int((out.t[r0:r1] != ref).sum())
        assert bad == 0, f"rows {r0} .. {r1}: {bad} entries differ, first rows {(r0 + (out.t[r0:r1] != ref).any(1).nonzero()[:4].flatten()).tolist()}"
        del ref
    print("adjoint past the cap: 0 entries differ")
    _peak_ok("adjoint past the cap", base)


# --------------------------------------------------------------------------------------------------------------- refusals
class Call:
    """An entry point with a full set of valid arguments by name; call(**overrides) -> its return code. `outs`: every buffer it could
    write."""

    def __init__(self, fn, names, args, outs):
        self.fn, self.names, self.args, self.outs = fn, names, args, outs

    def __call__(self, **o):
        assert set(o) <= set(self.names), o
        a = dict(self.args, **o)
        return self.fn(*[a[n] for n in self.names])

    def refused(self, want, **o):
        rc = self(**o)
        assert rc == want, (o, rc, want)

    def untouched(self):
        torch.cuda.synchronize()
        return all(x.untouched() for x in self.outs)


def _fwd_call(lib, dev, dtype, na, M=17, H=256, T=7):
    inp = L.fwd_inputs("exact", M, H, na, 1, dtype)
    ins = {"qkv": In(inp["qkv"], 3 * H + 8, dev, 0.0), "tT": In(inp["tT"], M + 3, dev, 3.0), "cs": In(L.quarter_turns(T), L.HD, dev, NAN)}
    ins.update({n: In(inp[n], 8, dev, 0.0, more_rows=1) for n in ("Bq", "Bv", "Bk")[:na]})
    outs = [Out(M, H, H + 8, dtype, dev) for _ in range(3)]
    names = ["qkv", "ld_qkv", "tT", "ldt", "Bq", "Bv"] + (["Bk"] if na == 3 else []) + ["ldb", "cs", "q", "k", "v", "ldo", "M", "H", "d", "T", "scale", "stream"]
    args = dict({n: i.ptr for n, i in ins.items()}, ld_qkv=3 * H + 8, ldt=M + 3, ldb=8, q=outs[0].ptr, k=outs[1].ptr, v=outs[2].ptr, ldo=H + 8,
                M=M, H=H, d=L.HD, T=T, scale=2.0, stream=_s())
    c = Call(_fn(lib, "haff_lora_qkv3_rope_fwd" if na == 3 else "haff_lora_qkv_rope_fwd", dtype), names, args, outs)
    c.keep = ins
    return c


@pytest.mark.parametrize("dtype", L.HALF, ids=_id)
@pytest.mark.parametrize("na", (2, 3))
def test_forward_refusals(dev, na, dtype):
    """null operands one at a time, M / T / H <= 0, d != 128, H % 128, ldb != 8, leading dimensions below their minimum or (where 16-byte
    accesses need it) no multiple of 8, every 16-byte operand one element off: the documented code, and q, k, v untouched"""
    c = _fwd_call(_lib(), dev, dtype, na)
    H, M = c.args["H"], c.args["M"]
    ptrs = ["qkv", "tT", "Bq", "Bv", "cs", "q", "k", "v"] + (["Bk"] if na == 3 else [])
    for n in ptrs:
        c.refused(BAD_ARG, **{n: None})
    for kw in (dict(M=0), dict(M=-1), dict(T=0), dict(T=-7), dict(H=0), dict(H=-128)):
        c.refused(BAD_ARG, **kw)
    for kw in (dict(d=64), dict(d=256), dict(H=192, ld_qkv=3 * H + 8), dict(H=8), dict(ldb=16), dict(ldb=0)):
        c.refused(UNSUPPORTED, **kw)
    for kw in (dict(ld_qkv=3 * H - 8), dict(ld_qkv=3 * H + 4), dict(ldo=H - 8), dict(ldo=H + 4), dict(ldt=M - 1), dict(ldt=0)):
        c.refused(BAD_ARG, **kw)
    for n in ptrs:
        if n != "tT":       # t^T is read with scalar loads: no alignment rule
            c.refused(BAD_ARG, **{n: c.args[n] + (4 if n == "cs" else 2)})
    assert c.untouched()
    assert c() == 0         # and the unmodified call is accepted


@pytest.mark.parametrize("dtype", L.HALF, ids=_id)
def test_adjoint_refusals(dev, dtype):
    lib, M, H, T = _lib(), 17, 256, 7
    grads = L.bwd_inputs("exact", M, H, 1, dtype)
    ins = [In(g, H + 8, dev, 0.0, more_rows=1) for g in grads] + [In(L.quarter_turns(T), L.HD, dev, NAN)]
    out = Out(M, 3 * H, 3 * H + 8, dtype, dev)
    names = ["dq", "dk", "dv", "ld_in", "cs", "dqkv", "ld_out", "M", "H", "d", "T", "stream"]
    c = Call(_fn(lib, "haff_lora_qkv_rope_bwd", dtype), names, dict(dq=ins[0].ptr, dk=ins[1].ptr, dv=ins[2].ptr, ld_in=H + 8, cs=ins[3].ptr, dqkv=out.ptr,
                                                                   ld_out=3 * H + 8, M=M, H=H, d=L.HD, T=T, stream=_s()), [out])
    for n in ("dq", "dk", "dv", "cs", "dqkv"):
        c.refused(BAD_ARG, **{n: None})
        c.refused(BAD_ARG, **{n: c.args[n] + (4 if n == "cs" else 2)})
    for kw in (dict(M=0), dict(M=-1), dict(T=0), dict(T=-1), dict(H=0), dict(H=-128), dict(ld_in=H - 8), dict(ld_in=H + 4), dict(ld_out=3 * H - 8),
               dict(ld_out=3 * H + 4)):
        c.refused(BAD_ARG, **kw)
    for kw in (dict(d=64), dict(d=130), dict(H=192), dict(H=64)):
        c.refused(UNSUPPORTED, **kw)
    assert c.untouched()
    assert c() == 0


def _dx_call(lib, dev, dtype, stem, M=17, Kd=256):
    na = 3 if stem == "haff_lora_dx3" else 2
    inp = L.dx_inputs("exact", M, Kd, na, 3, 1, dtype)
    ins = {"dtT": In(inp["dtT"], M + 3, dev, 3.0), "A": In(inp["A"], Kd + 3, dev, 0.0)}
    ins.update({n: In(k, Kd + 8, dev, 0.0, more_rows=1) for n, k in zip(("keep_q", "keep_v", "keep_k"), inp["keeps"])})
    out = Out(M, Kd, Kd + 8, dtype, dev, body=inp["dx0"].to(dev))
    masks = {"haff_lora_dx": ["keep_q"], "haff_lora_dx2": ["keep_q", "keep_v"], "haff_lora_dx3": ["keep_q", "keep_v", "keep_k"]}[stem]
    names = ["dtT", "ldt", "A", "lda"] + masks + ["ldk", "dx", "ldx", "accumulate", "M", "K", "scale", "stream"]
    args = dict({n: ins[n].ptr for n in ["dtT", "A"] + masks}, ldt=M + 3, lda=Kd + 3, ldk=Kd + 8, dx=out.ptr, ldx=Kd + 8, accumulate=1, M=M, K=Kd,
                scale=2.0, stream=_s())
    c = Call(_fn(lib, stem, dtype), names, args, [out])
    c.keep, c.masks = ins, masks
    return c


@pytest.mark.parametrize("dtype", L.HALF, ids=_id)
@pytest.mark.parametrize("stem", ("haff_lora_dx", "haff_lora_dx2", "haff_lora_dx3"), ids=lambda s: s[10:])
def test_dx_refusals(dev, stem, dtype):
    """null dtT / A / dx, M / K <= 0, K % 128, ldt < M, lda < K, ldx and ldk below K or no multiple of 8, dx and every mask one element
    off; dx2 with either mask null; dx3 with keep_v and no keep_k, with keep_v and no keep_q, with keep_k and no keep_v"""
    c = _dx_call(_lib(), dev, dtype, stem)
    M, Kd = c.args["M"], c.args["K"]
    for n in ("dtT", "A", "dx"):
        c.refused(BAD_ARG, **{n: None})
    for kw in (dict(M=0), dict(M=-1), dict(K=0), dict(K=-128), dict(ldt=M - 1), dict(lda=Kd - 1), dict(ldx=Kd - 8), dict(ldx=Kd + 4), dict(ldk=Kd - 8),
               dict(ldk=Kd + 4), dict(dx=c.args["dx"] + 2)):
        c.refused(BAD_ARG, **kw)
    for n in c.masks:
        c.refused(BAD_ARG, **{n: c.args[n] + 2})
    for kw in (dict(K=192), dict(K=64), dict(K=200)):
        c.refused(UNSUPPORTED, **kw)
    if stem == "haff_lora_dx2":
        c.refused(BAD_ARG, keep_q=None)
        c.refused(BAD_ARG, keep_v=None)
        c.refused(BAD_ARG, keep_q=None, keep_v=None)
    if stem == "haff_lora_dx3":
        c.refused(BAD_ARG, keep_k=None)                  # keep_v and no keep_k
        c.refused(BAD_ARG, keep_q=None)                  # keep_v (and keep_k) and no keep_q
        c.refused(BAD_ARG, keep_v=None)                  # keep_k and no keep_v
        c.refused(BAD_ARG, keep_q=None, keep_v=None)     # keep_k alone
    assert c.untouched()
    assert c() == 0


@pytest.mark.parametrize("dtype", L.HALF, ids=_id)
def test_tn_refusals(dev, dtype):
    """R not 8 or 16, j_valid 0 or R + 1, odd N, odd ldb, ldb < N, lds no multiple of 8 or below roundup(M, 16), a workspace one value short
    of haff_lora_tn_workspace_elems, ldo below the layout's minimum, null operands, sizes <= 0, sT / big off their 16 / 4 bytes"""
    lib, M, N, Rr = _lib(), 65, 130, 16
    inp = L.tn_inputs("exact", M, N, Rr, 1, dtype)
    sT_in, big_in = In(inp["sT"], 88, dev, 3.0, more_rows=1), In(inp["big"], N + 2, dev, 5.0, more_rows=1)
    n_ws = lib.haff_lora_tn_workspace_elems(M, Rr, N)
    assert n_ws == 2 * Rr * N
    ws, out = Out(1, n_ws, n_ws, F32, dev), Out(N, N, N + 8, F32, dev)
    names = ["sT", "lds", "R", "big", "ldb", "M", "N", "ws", "n_ws", "out", "ldo", "out_f32", "transposed", "j_valid", "scale", "stream"]
    c = Call(_fn(lib, "haff_lora_tn", dtype), names, dict(sT=sT_in.ptr, lds=88, R=Rr, big=big_in.ptr, ldb=N + 2, M=M, N=N, ws=ws.ptr, n_ws=n_ws, out=out.ptr,
                                                          ldo=N + 8, out_f32=1, transposed=0, j_valid=Rr, scale=2.0, stream=_s()), [ws, out])
    for out_f32 in (1, 0):
        for n in ("sT", "big", "ws", "out"):
            c.refused(BAD_ARG, out_f32=out_f32, **{n: None})
        for kw in (dict(M=0), dict(M=-1), dict(N=0), dict(N=-2), dict(j_valid=0), dict(j_valid=Rr + 1), dict(R=8, j_valid=9), dict(N=129), dict(ldb=N + 1),
                   dict(ldb=N - 2), dict(lds=84), dict(lds=72), dict(lds=64), dict(n_ws=n_ws - 1), dict(n_ws=0), dict(ldo=N - 2),
                   dict(transposed=1, ldo=Rr - 1), dict(transposed=1, j_valid=5, ldo=4), dict(sT=c.args["sT"] + 2), dict(sT=c.args["sT"] + 8),
                   dict(big=c.args["big"] + 2)):
            c.refused(BAD_ARG, out_f32=out_f32, **kw)
        for kw in (dict(R=4, j_valid=4), dict(R=12, j_valid=8), dict(R=32), dict(R=15, j_valid=8)):
            c.refused(UNSUPPORTED, out_f32=out_f32, **kw)
    assert c.untouched()
    for args, want in (((0, 8, 8), BAD_ARG), ((8, 0, 8), BAD_ARG), ((8, 8, 0), BAD_ARG), ((1025, 16, 130), 9 * 16 * 130)):
        assert lib.haff_lora_tn_workspace_elems(*args) == want, args
    assert c() == 0
