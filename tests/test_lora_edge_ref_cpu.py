"""The restatements of tests/lora_edge_ref.py checked on their own, without a GPU: against torch autograd of the definition at
float64; that the exact family is exact (its asserted maxima, the fp32 evaluation == float64, every value storable in bf16 and
f16); that every deliberate mistake misses its criterion (== on the exact family, the bound on the Gauss family), each ratio
printed; that a second correct evaluation in the kernels' own order stays inside the bound; and which of the mistakes the
criterion of the node-level tests (max|err| <= 3e-2 max|ref|) lets through — the measured statement of the gap the edge tests
close."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_edge_ref as R   # noqa: E402
import lora_edge_ref as L   # noqa: E402

F32, F64, BF16, F16 = R.F32, R.F64, R.BF16, R.F16
M_, H_, T_ = 100, 384, 7       # the mistakes are shown at seven 16-row tiles (the last of 4 rows), three heads, a position that wraps
OLD_PASSES = []


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("mistakes the node-level criterion max|err| <= 3e-2 max|ref| passes: " + (", ".join(OLD_PASSES) if OLD_PASSES else "none"))


def _fwd_args(inp, cs, T, H):
    return (inp["qkv"], inp["tT"], inp["Bq"], inp["Bv"], inp["Bk"], cs, T, H, inp["scale"])


def _dx_args(inp, nmasks_used, accumulate, na):
    return (inp["dtT"], inp["A"], inp["keeps"][:nmasks_used], inp["dx0"] if accumulate else None, inp["scale"], na)


# ------------------------------------------------------------------------------------------- against the definition at float64
@pytest.mark.parametrize("na", (2, 3))
@pytest.mark.parametrize("M,T", ((1, 1), (17, 7), (100, 100), (100, 7)))
def test_forward_and_adjoint_against_the_definition(M, T, na):
    """q, k, v against train_edge_ref.rope (written from the reference's rotate_half on split halves) of the adapted projections;
    the adjoint against autograd of that rotation"""
    H = 384
    inp = L.fwd_inputs("gauss", M, H, na, M + na, BF16)
    cs = L.angle_table(T)
    q, k, v = L.qkv_rope_fwd(*_fwd_args(inp, cs, T, H))
    x, t, s = inp["qkv"].double(), inp["tT"].double(), inp["scale"]
    rope = lambda z: R.rope(z, cs[:T], T, H // 128, 128, 0, False)   # noqa: E731
    q0 = x[:, :H] + s * (t[0:8].T @ inp["Bq"].double().T)
    k0 = x[:, H:2 * H] + (s * (t[16:24].T @ inp["Bk"].double().T) if na == 3 else 0.0)
    assert torch.allclose(q, rope(q0), rtol=0, atol=1e-12) and torch.allclose(k, rope(k0), rtol=0, atol=1e-12)
    assert torch.allclose(v, x[:, 2 * H:] + s * (t[8:16].T @ inp["Bv"].double().T), rtol=0, atol=1e-12)
    dq, dk, dv = L.bwd_inputs("gauss", M, H, M, BF16)
    got = L.qkv_rope_bwd(dq, dk, dv, cs, T, H)
    for i, up in enumerate((dq, dk)):
        vjp = R.autograd_of(rope, torch.zeros((M, H)), up)
        assert torch.allclose(got[:, i * H:(i + 1) * H], vjp, rtol=0, atol=1e-12)
    assert torch.equal(got[:, 2 * H:], dv.double())


@pytest.mark.parametrize("na,nmasks", ((2, 0), (2, 1), (2, 2), (3, 0), (3, 1), (3, 3)))
def test_dx_against_autograd(na, nmasks):
    """dx = the gradient with respect to x of sum_a scale ((x o keep_a) A_a^T) . dt_a, plus dx0"""
    M, Kd = 37, 256
    inp = L.dx_inputs("gauss", M, Kd, na, nmasks, 3 * na + nmasks, BF16)
    keeps = [k.double() for k in inp["keeps"]]

    def fn(x):
        tot = 0.0
        for a in range(na):
            keep = keeps[a] if nmasks == na else (keeps[0] if nmasks == 1 else 1.0)
            tot = tot + inp["scale"] * (((x * keep) @ inp["A"][8 * a:8 * a + 8].double().T) * inp["dtT"][8 * a:8 * a + 8].double().T).sum()
        return tot
    grad = R.autograd_of(fn, torch.zeros((M, Kd)), torch.tensor(1.0))
    assert torch.allclose(L.dx(*_dx_args(inp, nmasks, False, na)), grad, rtol=0, atol=1e-12)
    assert torch.allclose(L.dx(*_dx_args(inp, nmasks, True, na)), grad + inp["dx0"].double(), rtol=0, atol=1e-12)


@pytest.mark.parametrize("M", L.TN_M)
def test_tn_against_the_product_and_geometry(M):
    rpb, nb = L.tn_geometry(M)
    assert rpb % 64 == 0 and rpb >= 64 and nb <= 17 and (nb - 1) * rpb < M <= nb * rpb
    assert rpb == max(64, (((M + 15) // 16 + 63) // 64) * 64)          # lora_tn_rows_per_block, written out once more
    inp = L.tn_inputs("gauss", M, 130, 16, M, BF16)
    ref = inp["scale"] * (inp["sT"].double()[:13, :M] @ inp["big"].double())
    assert torch.allclose(L.lora_tn(inp["sT"], inp["big"], M, inp["scale"], 13, 0), ref, rtol=0, atol=1e-9)
    assert torch.equal(L.lora_tn(inp["sT"], inp["big"], M, inp["scale"], 13, 1), L.lora_tn(inp["sT"], inp["big"], M, inp["scale"], 13, 0).T)


def test_shape_lists_sit_on_the_edges():
    assert L.tn_geometry(1024) == (64, 16) and L.tn_geometry(1025) == (128, 9) and L.tn_edge_rows(1025)[-2:] == [1023, 1024]
    M, H = L.BIG_FWD["M"], L.BIG_FWD["H"]
    cap = -(-L.FWD_CAP // (H // 128))
    assert cap == 64 and -(-M // 16) > 4 * cap and -(-4099 // 16) > 4 * cap >= -(-4096 // 16)
    assert L.BIG_BWD["M"] * (L.BIG_BWD["H"] // 128) * 8 > L.BWD_CAP >= 524288 * 8
    assert 64 in L.ROWS and 65 in L.ROWS        # gridDim.y 1 -> 2
    for lay in L.LAYOUTS:
        d = L.lds(lay, 17, 384)
        assert d["ldt"] >= 17 and d["lda"] >= 384 and d["w"] % 8 == 0 and d["w3"] % 8 == 0
    assert L.lds("odd", 17, 384)["ldt"] % 2 == 0 and L.lds("tight", 17, 384)["ldt"] % 2 == 1 and L.lds("odd", 17, 384)["lda"] % 2 == 1


# ----------------------------------------------------------------------------------------------------------- the exact family
def _is_exact(name, outs32, outs64):
    for o32, o64 in zip(outs32, outs64):
        big = float(o64.abs().max())
        assert big <= L.EXACT_MAX and torch.equal(o64, o64.round()), (name, big)
        assert torch.equal(o32.double(), o64), name                       # the fp32 evaluation loses nothing
        for d in L.HALF:
            assert torch.equal(o64.to(d).double(), o64), (name, d)        # and the 16-bit store neither
    return max(float(o.abs().max()) for o in outs64)


@pytest.mark.parametrize("family", ("exact", "probe"))
def test_exact_family_is_exact(family):
    worst = {}
    for na in (2, 3):
        for M, T in ((100, 7), (65, 1)):
            inp = L.fwd_inputs(family, M, H_, na, M + na, BF16)
            cs = L.quarter_turns(T)
            a = _fwd_args(inp, cs, T, H_)
            worst["fwd"] = max(worst.get("fwd", 0), _is_exact("fwd", L.qkv_rope_fwd(*a, dt=F32), L.qkv_rope_fwd(*a)))
            ab = L.qkv_rope_fwd(*a, absolute=True)                         # the sums of absolute terms bound every partial sum
            assert max(float(z.max()) for z in ab) <= (104 if family == "exact" else 133)
        for nm in (0, 1, na):
            inp = L.dx_inputs(family, M_, 384, na, nm, na + nm, BF16)
            for acc in (False, True):
                a = _dx_args(inp, nm, acc, na)
                worst["dx"] = max(worst.get("dx", 0), _is_exact("dx", (L.dx(*a, dt=F32),), (L.dx(*a),)))
                assert float(L.dx(*a, absolute=True).max()) <= (200 if family == "exact" else 256)
    if family == "exact":
        dq, dk, dv = L.bwd_inputs("exact", M_, H_, 5, BF16)
        cs = L.quarter_turns(T_)
        worst["bwd"] = _is_exact("bwd", (L.qkv_rope_bwd(dq, dk, dv, cs, T_, H_, dt=F32),), (L.qkv_rope_bwd(dq, dk, dv, cs, T_, H_),))
        assert worst["bwd"] <= 64
        for M in L.TN_M:
            for N in L.TN_N:
                inp = L.tn_inputs("exact", M, N, 16, M + N, BF16)
                a = (inp["sT"], inp["big"], M, inp["scale"], 16, 0)
                worst["tn"] = max(worst.get("tn", 0), _is_exact("tn", (L.lora_tn(*a, dt=F32),), (L.lora_tn(*a),)))
                assert float(L.lora_tn(*a, absolute=True).max()) <= 2.0 ** 24
    print(f"{family} family, largest |result|: " + ", ".join(f"{k} {v:.0f}" for k, v in sorted(worst.items())))


def test_quarter_turn_table():
    cs = L.quarter_turns(7)
    co, si = cs[:7, :64], cs[:7, 64:]
    assert torch.equal(co * co + si * si, torch.ones((7, 64))) and torch.equal(co * si, torch.zeros((7, 64)))
    assert bool(torch.isnan(cs[7:]).all()) and cs.shape == (9, 128)
    assert not torch.equal(cs[0], cs[1]) and not torch.equal(co[:, 0], co[:, 1])     # varies with the position and the column pair
    assert len({(float(a), float(b)) for a, b in zip(co.reshape(-1), si.reshape(-1))}) == 4


# ------------------------------------------------------------------------------------------------------------ the mistakes
def _judge(name, wrong_exact, right_exact, wrong_gauss, expect_gauss, dtype):
    """One mistake on both families: the exact outputs must differ from the restatement's, the Gauss outputs must leave the bound
    in at least one output. Records whether the node-level criterion passes the Gauss outputs."""
    if wrong_exact is not None:
        same = all(torch.equal(torch.nan_to_num(w.to(dtype).double(), nan=1e300), torch.nan_to_num(r.to(dtype).double(), nan=1e300))
                   for w, r in zip(wrong_exact, right_exact))
        print(f"{name}: exact family {'EQUAL' if same else 'differs'}")
        assert not same, f"{name}: the exact family does not see it"
    ratios = [R.ratio(w.to(dtype), ref, bnd) for w, (ref, bnd) in zip(wrong_gauss, expect_gauss)]
    old = all(L.old_criterion(w.to(dtype), ref) for w, (ref, _) in zip(wrong_gauss, expect_gauss))
    print(f"{name}: Gauss |err| / bound " + ", ".join(f"{r:.3g}" for r in ratios) + f"; node-level criterion {'PASSES' if old else 'fails'}")
    assert max(ratios) > 1.0, f"{name}: inside the bound"
    if old:
        OLD_PASSES.append(name)


@pytest.mark.parametrize("dtype", L.HALF, ids=lambda d: L.IDS[d])
def test_forward_mistakes(dtype):
    cs_e, cs_g = L.quarter_turns(T_), L.angle_table(T_)
    e, g = L.fwd_inputs("exact", M_, H_, 3, 1, dtype), L.fwd_inputs("gauss", M_, H_, 3, 2, dtype)
    ae, ag = _fwd_args(e, cs_e, T_, H_), _fwd_args(g, cs_g, T_, H_)
    right, exp = L.qkv_rope_fwd(*ae), L.expect(L.qkv_rope_fwd, ag, (dtype,) * 3)
    for r, (ref, bnd) in zip(L.qkv_rope_fwd(*ag, dt=F32), exp):        # the criterion passes the correct evaluation
        assert R.ratio(r.to(dtype), ref, bnd) <= 1.0
    for m in L.FWD_MISTAKES:
        _judge(f"forward {m} {L.IDS[dtype]}", L.qkv_rope_fwd(*ae, **{m: True}), right, L.qkv_rope_fwd(*ag, **{m: True}), exp, dtype)
    # the probe family sees a misplaced rank on its own: rank 3 dropped, the v ranks taken from the q rows
    p = L.fwd_inputs("probe", M_, H_, 3, 3, dtype)
    ap = _fwd_args(p, cs_e, T_, H_)
    for m in ("drop_rank", "v_from_q_rows", "k_after_rope"):
        assert not all(torch.equal(a, b) for a, b in zip(L.qkv_rope_fwd(*ap, **{m: True}), L.qkv_rope_fwd(*ap))), m
    # k only: an update landing on q or v from the k ranks would show against Bq, Bv != 0
    ko = L.fwd_inputs("exact", M_, H_, 3, 4, dtype, k_only=True)
    q, k, v = L.qkv_rope_fwd(*_fwd_args(ko, cs_e, T_, H_))
    assert torch.equal(v, ko["qkv"].double()[:, 2 * H_:]) and float(ko["Bq"].abs().max()) > 0
    assert not torch.equal(k, L._rot(ko["qkv"][:, H_:2 * H_], cs_e, T_, False, F64))
    # the two buffer-level mistakes: == on the whole sentinel-filled buffer sees them, the node-level criterion (which looks at
    # rows < M only) cannot see the first
    full = L.embed(right[0], M_ + 3, H_ + 8, dtype)
    assert not torch.equal(L.embed(right[0], M_ + 3, H_ + 8, dtype, clamp_row_written=True), full)
    assert not torch.equal(L.embed(right[0], M_ + 3, H_ + 8, dtype, skip_tile=6), full)
    if dtype == BF16:
        OLD_PASSES.append("forward / adjoint / dx clamp_row_written (row M is not looked at)")


@pytest.mark.parametrize("dtype", L.HALF, ids=lambda d: L.IDS[d])
def test_adjoint_mistakes(dtype):
    cs_e, cs_g = L.quarter_turns(T_), L.angle_table(T_)
    e, g = L.bwd_inputs("exact", M_, H_, 1, dtype), L.bwd_inputs("gauss", M_, H_, 2, dtype)
    right = (L.qkv_rope_bwd(*e, cs_e, T_, H_),)
    exp = L.expect(L.qkv_rope_bwd, (*g, cs_g, T_, H_), dtype)
    assert R.ratio(L.qkv_rope_bwd(*g, cs_g, T_, H_, dt=F32).to(dtype), *exp[0]) <= 1.0
    for m in L.BWD_MISTAKES:
        _judge(f"adjoint {m} {L.IDS[dtype]}", (L.qkv_rope_bwd(*e, cs_e, T_, H_, **{m: True}),), right,
               (L.qkv_rope_bwd(*g, cs_g, T_, H_, **{m: True}),), exp, dtype)


DX_CASES = {"swap_qv": ((2, 2), (3, 3)), "swap_vk": ((3, 3),), "mask_wrong_ranks": ((2, 2), (3, 3)), "drop_rank": ((2, 0), (2, 1), (3, 3)),
            "no_k_lanes": ((3, 0), (3, 1), (3, 3)), "ignore_accumulate": ((2, 1), (3, 3)), "skip_tile": ((2, 1), (3, 3)),
            "double_tile": ((2, 1), (3, 3))}


@pytest.mark.parametrize("dtype", L.HALF, ids=lambda d: L.IDS[d])
@pytest.mark.parametrize("Kd", (384, 4096))
def test_dx_mistakes(dtype, Kd):
    """Every mistake with every mask arrangement it applies to, with accumulate = 1 on a dx0 of the frozen adjoint's size (and
    accumulate = 0 for the ones that concern it). At K = 4096 the adapter term is the few percent of max|dx| the trainer sees."""
    M = M_ if Kd == 384 else 36
    for m, cases in DX_CASES.items():
        for na, nm in cases:
            e, g = L.dx_inputs("exact", M, Kd, na, nm, 10 + na + nm, dtype), L.dx_inputs("gauss", M, Kd, na, nm, 20 + na + nm, dtype)
            for acc in ((True, False) if m in ("ignore_accumulate", "skip_tile") else (True,)):
                ae, ag = _dx_args(e, nm, acc, na), _dx_args(g, nm, acc, na)
                exp = L.expect(L.dx, ag, dtype)
                assert R.ratio(L.dx(*ag, dt=F32).to(dtype), *exp[0]) <= 1.0
                _judge(f"dx {m} na {na} masks {nm} accumulate {int(acc)} K {Kd} {L.IDS[dtype]}", (L.dx(*ae, **{m: True}),), (L.dx(*ae),),
                       (L.dx(*ag, **{m: True}),), exp, dtype)
    p = L.dx_inputs("probe", M, Kd, 3, 3, 7, dtype)
    for m in ("drop_rank", "no_k_lanes", "swap_qv", "swap_vk"):
        assert not torch.equal(L.dx(*_dx_args(p, 3, True, 3), **{m: True}), L.dx(*_dx_args(p, 3, True, 3))), m


@pytest.mark.parametrize("dtype", L.HALF, ids=lambda d: L.IDS[d])
def test_tn_mistakes(dtype):
    for M, N in ((1025, 130), (65, 2), (17, 126)):
        e, g = L.tn_inputs("exact", M, N, 16, M, dtype), L.tn_inputs("gauss", M, N, 16, M + 1, dtype)
        for out_dtype in (F32, dtype):
            ae, ag = (e["sT"], e["big"], M, e["scale"], 13, 0), (g["sT"], g["big"], M, g["scale"], 13, 0)
            exp = L.expect(L.lora_tn, ag, out_dtype)
            assert R.ratio(L.lora_tn(*ag, dt=F32).to(out_dtype), *exp[0]) <= 1.0
            for m in L.TN_MISTAKES:
                _judge(f"tn {m} M {M} N {N} out {R.IDS[out_dtype]} {L.IDS[dtype]}", (L.lora_tn(*ae, **{m: True}),), (L.lora_tn(*ae),),
                       (L.lora_tn(*ag, **{m: True}),), exp, out_dtype)


# --------------------------------------------------------------------------------------- a second evaluation, in the kernels' order
@pytest.mark.parametrize("dtype", L.HALF, ids=lambda d: L.IDS[d])
def test_kernel_order_stays_inside_the_bound(dtype):
    """fp32, the ranks one after the other (the MFMA's k index), scale *, the add, the rotation, one rounding to the 16-bit type;
    tn per wave, step and row block: every output inside the bound of the float64 reference"""
    worst = {}

    def note(name, got, ref, bnd):
        r = R.ratio(got, ref, bnd)
        worst[name] = max(worst.get(name, 0.0), r)
        assert r <= 1.0, (name, r)
    for M, T in ((100, 7), (17, 17), (1, 1)):
        cs = L.angle_table(T)
        for na in (2, 3):
            g = L.fwd_inputs("gauss", M, H_, na, 30 + M + na, dtype)
            a = _fwd_args(g, cs, T, H_)
            for n, got, (ref, bnd) in zip("qkv", L.qkv_rope_fwd_ordered(*a, dtype), L.expect(L.qkv_rope_fwd, a, (dtype,) * 3)):
                note(f"forward {n}", got, ref, bnd)
            for nm in (0, 1, na):
                for Kd in (384, 4096) if M == 17 else (384,):
                    d = L.dx_inputs("gauss", M, Kd, na, nm, 40 + M + na + nm, dtype)
                    for acc in (False, True):
                        ad = _dx_args(d, nm, acc, na)
                        note("dx", L.dx_ordered(*ad, dtype), *L.expect(L.dx, ad, dtype)[0])
    for M, N, Rr in ((1039, 130, 16), (65, 126, 8), (1, 2, 8)):
        g = L.tn_inputs("gauss", M, N, Rr, M + N, dtype)
        for out_dtype in (F32, dtype):
            a = (g["sT"], g["big"], M, g["scale"], Rr - 3, 0)
            note(f"tn {R.IDS[out_dtype]}", L.lora_tn_ordered(g["sT"], g["big"], M, g["scale"], Rr - 3, out_dtype), *L.expect(L.lora_tn, a, out_dtype)[0])
    print(f"kernel-order evaluation {L.IDS[dtype]}, worst |err| / bound: " + ", ".join(f"{k} {v:.4f}" for k, v in sorted(worst.items())))
