"""tests/attn_edge_ref.py on its own, before any GPU sees its inputs: for every case list the GPU file runs, every builder's margin
assertion holds (the builders assert it as they build), the float64 reference of a one-hot case IS the chosen V row, a second correct
evaluation (fp32, the kernels' documented roundings, 64 keys at a time with a running maximum) stays inside the format-derived bound
on every row of every case, and every mistake flag that applies to a kernel family misses the bound by 10x or more on at least one
case of that family (the mistakes are evaluated on the short cases of each list: up to 30 window items, the decode shapes of up to
16 heads, head 0 of the fused-table case; margins and the blocked evaluation run on every case). Every query row is compared; padded window positions, which no caller reads, are the only rows left out."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import attn_edge_ref as A   # noqa: E402

BF16, F16, F32 = A.BF16, A.F16, A.F32
_id = lambda v: A.IDS.get(v, None)   # noqa: E731
CAUGHT = {}


@pytest.fixture(autouse=True)
def _fresh_caught():
    """every test, and each type of a parametrised one, has to catch its flags itself"""
    CAUGHT.clear()
    yield


def _u(family, dtype):
    return A.U16[dtype] if family in ("generic", "pp", "window") and dtype != F32 else A.U32


def _ratio(got, ref, c, family):
    bnd = A.bound(ref, c.vmax, c.q.dtype, _u(family, c.q.dtype))
    r = (got.double() - ref).abs() / bnd
    r = torch.where(torch.isnan(r), torch.full_like(r, A.INF), r)
    if c.is_pad is not None:
        r = r.permute(0, 2, 1, 3)[~c.is_pad]
    return float(r.max())


def _inside(c, family, what):
    ref = c.ref()
    if c.onehot:
        assert torch.equal(ref.to(c.q.dtype)[_rows(c)], c.v_choice()[_rows(c)]), f"{what}: the reference is not the chosen V row"
    r = _ratio(A.attn_blocked(c, family), ref, c, family)
    print(f"{family} {what}: blocked evaluation at {r:.3g} of the bound")
    assert r <= 1.0, f"{family} {what}: the blocked evaluation stands at {r:.3g} of the bound"
    return ref


def _rows(c):
    if c.is_pad is None:
        return slice(None)
    return (~c.is_pad)[:, None, :].expand(c.q.shape[:3])


def _flags(c, family, what, flags, ref=None, rebuild=None):
    """each flag's miss of the bound on this case, kept as the family's best"""
    ref = c.ref() if ref is None else ref
    for f in flags:
        if f in ("rel_row_plus1", "pad_as_zero"):
            wrong = rebuild(**{f: True}).ref()
        else:
            wrong = c.ref(**{f: True})
        r = _ratio(wrong, ref, c, family)
        CAUGHT[(family, f)] = max(CAUGHT.get((family, f), 0.0), r)


def _need(family, flags):
    for f in flags:
        r = CAUGHT.get((family, f), 0.0)
        print(f"{family}: {f} misses the bound by {r:.3g}x")
        assert r >= 10.0, f"{family}: {f} is not caught (best {r:.3g}x)"


# ---------------------------------------------------------------------------------------------------------------- generic
def generic_cases(dtype):
    """(name, Case) of every generic-kernel case of the GPU file"""
    for t in A.GENERIC_PLAIN:
        d, B, H, Nq, Nk, causal, p0 = t
        yield "qk-" + A.case_id(t), A.select_by_qk(B, H, Nq, Nk, d, Nq + Nk, dtype, bool(causal), p0)
        yield "pair-" + A.case_id(t), A.pair_inputs(B, H, Nq, Nk, d, Nq + Nk + 1, dtype, bool(causal), p0, first=64)
        if Nk > 81:
            yield "late-" + A.case_id(t), A.pair_inputs(B, H, Nq, Nk, d, Nq + Nk + 2, dtype, bool(causal), p0, late_jump=True, first=64)
    for t in A.GENERIC_BIAS3 + A.GENERIC_BIAS1 + A.GENERIC_BIAS2 + (A.GENERIC_BIAS2_SPLIT_KV,):
        d, B, H, Nq, Nk, S = t
        yield "bias-" + A.case_id(t), A.select_by_bias(B, H, Nq, Nk, d, S, Nq + S, dtype)


def ragged_case(dtype, pair=False, nan=False, d=64, H=3, nks=A.RAGGED_NK):
    B, Tmax = len(nks), max(nks)
    if pair:
        return A.ragged_poison(A.pair_inputs(B, H, 1, Tmax, d, 21, dtype, nk_rows=nks, first=64), nan)
    return A.ragged_poison(A.select_by_qk(B, H, 1, Tmax, d, 20, dtype, nk_rows=nks, choice=A.decode_choice(B, H, nks)), nan)


@pytest.mark.parametrize("dtype", A.HALF, ids=_id)
def test_generic(dtype):
    for name, c in generic_cases(dtype):
        ref = _inside(c, "generic", f"{name} {A.IDS[dtype]}")
        flags = ["key_plus1", "drop_last_key", "drop_key63", "next_head_v"]
        flags += ["mask_lt", "no_q_pos0"] if c.causal else []
        flags += ["swap_hw"] if c.relh is not None else []
        flags += ["no_rescale"] if c.jump is not None else []
        _flags(c, "generic", name, flags, ref)
    for pair in (False, True):
        for nan in (False, True):
            c = ragged_case(dtype, pair, nan)
            ref = _inside(c, "generic", f"ragged pair {pair} nan {nan} {A.IDS[dtype]}")
            _flags(c, "generic", "ragged", ["nk_plus1", "nk_of_batch0"], ref)
    _need("generic", ("swap_hw", "key_plus1", "drop_last_key", "drop_key63", "mask_lt", "no_q_pos0", "nk_plus1", "nk_of_batch0",
                      "next_head_v", "no_rescale"))


# ------------------------------------------------------------------------------------------------------------- ping-pong
def pp_cases(dtype):
    for B, H, Nq, nkt in A.PP_TABLES:
        yield f"bias-{B}-{H}-{Nq}-{nkt}", A.select_by_bias(B, H, Nq, 64 * nkt, 80, 64, Nq + nkt, dtype)
    for B, H, Nq, nkt, late in A.PP_PAIR:
        yield f"pair-{B}-{H}-{Nq}-{nkt}-{late}", A.pair_inputs(B, H, Nq, 64 * nkt, 80, Nq + nkt, dtype, late_jump=late, first=64, S=64)


@pytest.mark.parametrize("dtype", A.HALF, ids=_id)
def test_pingpong(dtype):
    for name, c in pp_cases(dtype):
        ref = _inside(c, "pp", f"{name} {A.IDS[dtype]}")
        flags = ["key_plus1", "drop_last_key", "drop_key63", "next_head_v"] + (["swap_hw"] if c.onehot else []) + (["no_rescale"] if c.jump is not None else [])
        _flags(c, "pp", name, flags, ref)
    _need("pp", ("swap_hw", "key_plus1", "drop_last_key", "drop_key63", "next_head_v", "no_rescale"))


def test_pingpong_fused_tables():
    """N = 4096, the H = 3 case the GPU file builds (its H = 1 launch is head 0 of it), in both types; the mistakes on head 0"""
    S = A.GLB_S
    c3 = A.select_by_tables_64(3, 5, BF16)
    for dtype in A.HALF:
        _inside(A.recast_tables_64(c3, dtype), "pp", f"fused tables H 3 {A.IDS[dtype]}")
    c = A.heads_of(c3, 1)
    ref = _inside(c, "pp", "fused tables H 1")
    _flags(c, "pp64", "fused tables", ["swap_hw", "key_plus1", "drop_key63"], ref)
    relh, relw = A.relpos_from_tables(c.q, c.tab_h, c.tab_w, S, rel_row_plus1=True)
    wrong = A.attn_ref(c.q, c.k, c.v, c.scale, relh=relh, relw=relw, S=S)
    CAUGHT[("pp64", "rel_row_plus1")] = _ratio(wrong, ref, c, "pp")
    _need("pp64", ("swap_hw", "rel_row_plus1", "key_plus1", "drop_key63"))
    for dtype in A.HALF:
        c = A.select_by_qk(1, 1, S * S, S * S, A.GLB_D, 9, dtype)
        c.S, c.relh, c.relw = S, torch.zeros((1, 1, S * S, S)), torch.zeros((1, 1, S * S, S))
        _inside(c, "pp", f"q.k on zero tables {A.IDS[dtype]}")


# ------------------------------------------------------------------------------------------------------------------ decode
@pytest.mark.parametrize("dtype", A.HALF, ids=_id)
def test_decode(dtype):
    for B, H, Tmax, nks in A.DECODE:
        for pair, nan in ((False, False), (False, True), (True, True)):
            c = A.decode_case(B, H, Tmax, nks, B + H, dtype, pair=pair, nan=nan)
            ref = _inside(c, "decode", f"B {B} H {H} pair {pair} nan {nan} {A.IDS[dtype]}")
            if H <= 16:     # the mistakes are shown on the two short shapes: a flag has to be caught once
                _flags(c, "decode", "", ["key_plus1", "drop_last_key", "nk_plus1", "nk_of_batch0", "next_head_v", "drop_last_wave"], ref)
        c = A.rope_case(B, H, Tmax, nks, B + H + 1, dtype)[0]
        _inside(c, "decode", f"rope B {B} H {H} {A.IDS[dtype]}")
    _need("decode", ("key_plus1", "drop_last_key", "nk_plus1", "nk_of_batch0", "next_head_v", "drop_last_wave"))


def test_rope_roundtrip():
    """rope_inv undoes rope to the table's fp32 rounding; the new K row the case carries is r16 of the float64 rotation"""
    cs = A.cos_sin_table(70, 128)
    x = A.rand((5, 3, 128), 1).double()
    pos = torch.tensor([0, 1, 17, 64, 69])[:, None]
    # the table is fp32, so cos^2 + sin^2 = 1 +- 2^-23: the round trip scales x by that
    assert float((A.rope_inv(A.rope(x, pos, cs), pos, cs) - x).abs().max()) < 4 * 2.0 ** -23 * float(x.abs().max())
    assert torch.equal(A.rope(x, torch.zeros((5, 1), dtype=torch.long), cs), x)
    c, qkv, k0, v0, _ = A.rope_case(3, 2, 70, (1, 17, 70), 3, BF16)
    for b, n in enumerate((1, 17, 70)):
        assert torch.equal(c.k[b, :, n - 1], c.k_rot64[b].to(BF16)) and torch.equal(c.v[b, :, n - 1], qkv[b, 2])
        assert bool(torch.isnan(k0[b, :, n - 1:]).all()) and torch.equal(k0[b, :, :n - 1], c.k[b, :, :n - 1])


# ------------------------------------------------------------------------------------------------------------------ window
def window_cases(dtype):
    for n_win, H in A.WINDOW_ITEMS:
        yield f"t14-{n_win}x{H}", A.select_by_tables_14(n_win, H, n_win, dtype), None
        yield f"qk-{n_win}x{H}", A.select_window_qk(n_win, H, n_win, dtype), None
    for grid, H in A.WINDOW_GRIDS:
        n_win = 2 * (-(-grid // 14)) ** 2
        yield f"t14-grid{grid}x{H}", A.select_by_tables_14(n_win, H, grid, dtype, grid), (lambda g=grid, n=n_win, h=H, **w: A.select_by_tables_14(n, h, g, dtype, g, **w))
        yield f"qk-grid{grid}x{H}", A.select_window_qk(n_win, H, grid, dtype, grid), (lambda g=grid, n=n_win, h=H, **w: A.select_window_qk(n, h, g, dtype, g, **w))


@pytest.mark.parametrize("dtype", A.HALF, ids=_id)
def test_window(dtype):
    for name, c, rebuild in window_cases(dtype):
        ref = _inside(c, "window", f"{name} {A.IDS[dtype]}")
        if c.q.shape[0] * c.q.shape[1] > 30:     # the mistakes are shown on the short item lists: a flag has to be caught once
            continue
        flags = ["key_plus1", "drop_last_key", "next_head_v"]
        if name.startswith("t14"):
            flags += ["swap_hw"]
            rb = rebuild or (lambda n=c.q.shape[0], h=c.q.shape[1], **w: A.select_by_tables_14(n, h, n, dtype, **w))
            _flags(c, "window", name, ["rel_row_plus1"], ref, rb)
        if rebuild is not None and c.is_pad.any():
            _flags(c, "window", name, ["pad_as_zero"], ref, rebuild)
        _flags(c, "window", name, flags, ref)
    _need("window", ("swap_hw", "rel_row_plus1", "key_plus1", "drop_last_key", "next_head_v", "pad_as_zero"))


def test_window_fill_geometry():
    """grid 15: the corner window of each image holds a single real token, the edge windows one real row / column; grid 14 and 28: no
    padded position at all"""
    qkv = torch.zeros((8, 196, 3, 1, 8))
    pad = torch.ones((3, 1, 8))
    full, is_pad = A.window_fill(qkv, 15, 14, pad)
    real = (~is_pad).sum(1).tolist()
    assert real == [196, 14, 14, 1] * 2
    assert bool((full[is_pad] == 1).all()) and bool((full[~is_pad] == 0).all())
    assert not bool(A.window_fill(qkv[:2], 14, 14, pad)[1].any()) and not bool(A.window_fill(qkv, 28, 14, pad)[1].any())
    assert (~A.window_fill(qkv, 20, 14, pad)[1]).sum(1).tolist() == [196, 84, 84, 36] * 2


# -------------------------------------------------------------------------------------------------------------------- fp32
def f32_cases():
    for t in A.F32_PLAIN + A.F32_FEW:
        d, B, H, Nq, Nk, causal, p0, _ = t
        yield "qk-" + A.case_id(t), A.select_by_qk(B, H, Nq, Nk, d, Nq + Nk, F32, bool(causal), p0)
    for t in A.F32_BIAS:
        d, B, H, Nq, Nk, causal, p0, S = t
        yield "bias-" + A.case_id(t), (A.causal_bias_case(d, B, H, Nq, Nk, p0, S, Nq, F32) if causal else A.select_by_bias(B, H, Nq, Nk, d, S, Nq, F32))
    for d, B, H, Tmax, nks in A.F32_RAGGED:
        for nan in (False, True):
            yield f"ragged-{d}-nan{nan}", ragged_case(F32, False, nan, d, H, nks)


def test_f32():
    for name, c in f32_cases():
        ref = _inside(c, "f32", name)
        flags = ["key_plus1", "drop_last_key", "next_head_v"] + (["mask_lt", "no_q_pos0"] if c.causal else []) + (["swap_hw"] if c.relh is not None else [])
        flags += ["nk_plus1", "nk_of_batch0"] if c.nk_rows is not None else []
        _flags(c, "f32", name, flags, ref)
    _need("f32", ("swap_hw", "key_plus1", "drop_last_key", "mask_lt", "no_q_pos0", "nk_plus1", "nk_of_batch0", "next_head_v"))


def test_bound_and_mistake_list():
    """the bound is the stated one: u |v| plus one ulp of the output format at |ref|"""
    ref = torch.tensor([1.0, 1.5, 0.75, 3.0, 0.0], dtype=torch.float64)
    assert A.ulp(ref, BF16).tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -8, 2.0 ** -6, 2.0 ** -133]
    assert A.ulp(ref, F16).tolist() == [2.0 ** -10, 2.0 ** -10, 2.0 ** -11, 2.0 ** -9, 2.0 ** -24]
    assert float(A.bound(ref[:1], torch.tensor([2.0]), BF16, A.U16[BF16])) == 2.0 ** -7 + 2.0 ** -7
    assert (A.U16[BF16], A.U16[F16], A.U32, A.GAIN, A.MARGIN) == (2.0 ** -8, 2.0 ** -11, 2.0 ** -22, 24.0, 160.0)
    assert len(A.MISTAKES) == 13 and len(set(A.MISTAKES)) == 13
