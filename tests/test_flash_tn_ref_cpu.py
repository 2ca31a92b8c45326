"""tests/flash_tn_ref.py on its own, without a GPU: gemm_tn against torch's float64 product, attn against float64 autograd of the
masked softmax definition and torch.logsumexp; a second correct evaluation in the kernels' block order (attn_blocked) inside the
per-row bound on every listed flash shape in both 16-bit types; every deliberate mistake outside that bound on the trap inputs, at
the smallest listed shape where the mistake can show; and for gemm_tn's exact inputs, one row dropped or counted twice at a slab or
split edge changes some entry by at least 1, which the GPU file's == cannot miss.

Worst ratio of attn_blocked to the bound over FLASH_SHAPES (trap inputs; printed by test_blocked_evaluation_meets_the_bound):
bf16 out 0.433, lse2 0.250, dq 0.302, dk 0.212, dv 0.261; f16 out 0.383, lse2 0.252, dq 0.289, dk 0.289, dv 0.285. The evaluation
the bound is built from stands at 1 / K = 0.25 by construction; the blocked one rounds its probabilities against the running
maximum and so draws other roundings of the same size. Without flash_tn_ref.delta_terms its dq stood at 1.07 (bf16, 130 x 130
causal) and 1.06 (f16, 130 x 70): see there. Every mistake stands between 9 (drop_query63, bf16 dk) and 2e4 times the bound in the
results it has to move."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import train_edge_ref as R   # noqa: E402
import flash_tn_ref as T   # noqa: E402

F32, F64, BF16, F16 = R.F32, R.F64, R.BF16, R.F16
WORST = {}


def _same(a, b, tol=1e-12):
    a, b = a.double(), b.double()
    assert (a - b).abs().max().item() <= tol * (b.abs().max().item() + 1e-30), (a - b).abs().max().item()


def _shape(Nq, Nk, causal, q_pos0):
    """the first listed shape with these lengths and mask"""
    return next(s for s in T.FLASH_SHAPES if s[2:6] == (Nq, Nk, causal, q_pos0))


# ------------------------------------------------------------------------------------------------------------------ gemm_tn
def test_gemm_tn_matches_torch():
    for M, (N1, N2) in ((65, (8, 8)), (257, (136, 264))):
        a, b = T.tn_gauss_inputs(M, N1, N2, M, BF16)
        assert torch.equal(T.gemm_tn(a, b), a.double().T @ b.double())
        ref, bnd = T.tn_expect(a, b, BF16)
        assert R.ratio(T.gemm_tn(a, b, F32).to(BF16), ref, bnd) <= 1.0
        assert R.ratio(T.gemm_tn(a, b, F32), ref, T.tn_expect(a, b, F32)[1]) <= 1.0


def test_tn_geometry_is_the_kernels():
    """one tile wants 64 splits, a split is a multiple of 64 rows and at least 256; 16 x 17 tiles want 2"""
    assert T.tn_geometry(70000, 256, 256) == (1152, 61)
    assert T.tn_geometry(64, 2048, 2056) == (256, 1)
    assert T.tn_geometry(1, 8, 8) == (256, 1)


@pytest.mark.parametrize("dtype", T.HALF, ids=lambda d: T.IDS[d])
def test_exact_inputs_are_exact_and_one_row_shows(dtype):
    """the fp32 row-by-row sum of the integer inputs equals the float64 product; a row dropped or doubled at the first or last row
    of a slab or split moves some entry by at least 1"""
    for M in T.TN_M:
        a, b = T.tn_exact_inputs(M, 8, 8, M, dtype)
        ref = T.gemm_tn(a, b)
        assert torch.equal(T.gemm_tn(a, b, F32).double(), ref) and float(ref.abs().max()) <= 16 * M < 2 ** 24
        for m in T.tn_edge_rows(M, 8, 8):
            assert float((T.gemm_tn(a, b, drop_row=m) - ref).abs().max()) >= 1.0, (M, m)
            assert float((T.gemm_tn(a, b, double_row=m) - ref).abs().max()) >= 1.0, (M, m)
    assert T.tn_edge_rows(20000, 8, 8) == [0, 63, 64, 319, 320, 19840, 19968, 19999]


# --------------------------------------------------------------------------------------------------------------- flash pair
def _autograd(q, k, v, do, scale, causal, q_pos0):
    """float64 autograd of the definition: softmax over the visible keys of scale q k^T, times v"""
    qd, kd, vd = (t.double().clone().requires_grad_(True) for t in (q, k, v))
    s = (qd @ kd.transpose(-1, -2)) * R.f32(scale)
    s = s.masked_fill(~T.visible(q.shape[2], k.shape[2], causal, q_pos0), -R.INF)
    out = torch.softmax(s, -1) @ vd
    out.backward(do.double())
    return out.detach(), torch.logsumexp(s.detach(), -1) / T.LN2, qd.grad, kd.grad, vd.grad


@pytest.mark.parametrize("shape", [s for s in T.FLASH_SHAPES if s[2] <= 131], ids=T.flash_id)
def test_attn_matches_autograd(shape):
    B, H, Nq, Nk, causal, q_pos0, _ = shape
    for inputs in (T.smooth_inputs(B, H, Nq, Nk, 3, BF16), T.trap_inputs(B, H, Nq, Nk, q_pos0, 3, F16)):
        for got, ref in zip(T.attn(*inputs, T.FLASH_SCALE, causal, q_pos0), _autograd(*inputs, T.FLASH_SCALE, causal, q_pos0)):
            _same(got, ref, 1e-10)


def test_trap_puts_weight_on_the_diagonal():
    """with the trap the last visible key of a causal row scores c |k|^2 scale = 0.3 * 128 / 11.3 = 3.4 above a typical key: e^3.4 = 30
    against about 100 keys of weight e^N(0,1), a share above 0.1; with plain Gaussians it holds about 1 / keys"""
    B, H, Nq, Nk, causal, q_pos0, _ = _shape(70, 133, 1, 63)
    for inputs, lo, hi in ((T.trap_inputs(B, H, Nq, Nk, q_pos0, 1, BF16), 0.1, 1.0), (T.smooth_inputs(B, H, Nq, Nk, 1, BF16), 0.0, 0.03)):
        q, k = inputs[0].double(), inputs[1].double()
        s = (q @ k.transpose(-1, -2)) * T.FLASH_SCALE
        p = torch.softmax(s.masked_fill(~T.visible(Nq, Nk, causal, q_pos0), -R.INF), -1)
        share = p[0, 0, torch.arange(Nq), torch.arange(Nq) + q_pos0].median().item()
        assert lo <= share <= hi, share


@pytest.mark.parametrize("r16", T.HALF, ids=lambda d: T.IDS[d])
def test_blocked_evaluation_meets_the_bound(r16):
    """a correct evaluation in the kernels' block order, fp32 accumulators and the documented roundings, is inside the per-row bound
    on every listed shape: the bound can be met"""
    worst = dict.fromkeys(T.RESULTS, 0.0)
    for shape in T.FLASH_SHAPES:
        B, H, Nq, Nk, causal, q_pos0, _ = shape
        inputs = T.trap_inputs(B, H, Nq, Nk, q_pos0, Nq + Nk, r16)
        exp = T.attn_expect(*inputs, T.FLASH_SCALE, causal, q_pos0, r16)
        got = T.attn_blocked(*inputs, T.FLASH_SCALE, causal, q_pos0, r16)
        for name, g, (ref, bnd) in zip(T.RESULTS, got, exp):
            r = R.ratio(g, ref, bnd)
            worst[name] = max(worst[name], r)
            assert r <= 1.0, (T.flash_id(shape), name, r)
    print("blocked evaluation, worst ratio to the bound,", T.IDS[r16], {n: round(w, 3) for n, w in worst.items()})


# mistake -> (Nq, Nk, causal, q_pos0) of the smallest listed shape where it can show, and the results it has to push out
MISTAKE_AT = {
    "mask_lt": ((63, 64, 1, 1), T.RESULTS),
    "mask_plus1": ((63, 64, 1, 1), ("out", "lse2", "dq", "dk", "dv")),
    "no_q_pos0": ((63, 64, 1, 1), T.RESULTS),
    "drop_key63": ((63, 64, 1, 1), T.RESULTS),                 # key 63 is the last query's diagonal
    "drop_query63": ((64, 64, 1, 0), ("dk", "dv")),             # query 63 is the only one that sees key 63
    "natural_lse": ((1, 1, 1, 0), ("lse2",)),
    "no_ds_scale": ((63, 64, 1, 1), ("dq", "dk")),
    "delta_other_head": ((64, 64, 1, 0), ("dq", "dk")),         # the smallest listed shape with H > 1
    "dq_first_block": ((127, 128, 0, 0), ("dq",)),              # queries 63 .. 126 have their two heavy keys in block 1 (at 65 x 65 the
                                                                # one key of block 1 holds nearly all of query 64's row, and dS -> 0 as P -> 1)
}


@pytest.mark.parametrize("r16", T.HALF, ids=lambda d: T.IDS[d])
@pytest.mark.parametrize("mistake", T.MISTAKES)
def test_every_mistake_misses_the_bound(mistake, r16):
    key, results = MISTAKE_AT[mistake]
    B, H, Nq, Nk, causal, q_pos0, _ = _shape(*key)
    inputs = T.trap_inputs(B, H, Nq, Nk, q_pos0, Nq + Nk, r16)
    exp = T.attn_expect(*inputs, T.FLASH_SCALE, causal, q_pos0, r16)
    wrong = T.attn(*inputs, T.FLASH_SCALE, causal, q_pos0, r16=r16, **{mistake: True})
    right = T.attn(*inputs, T.FLASH_SCALE, causal, q_pos0, r16=r16)
    for name, w, g, (ref, bnd) in zip(T.RESULTS, wrong, right, exp):
        rw, rg = R.ratio(w, ref, bnd), R.ratio(g, ref, bnd)
        print(f"{mistake} {T.IDS[r16]} {name}: wrong / bound = {rw:.3g} (right: {rg:.3g})")
        assert rg <= 0.26, (name, rg)        # the evaluation the bound is built from stands at 1 / K, its storage rounding included
        if name in results:
            assert rw > 1.0, f"{mistake} {name}: the wrong variant is inside the bound ({rw:.3g})"


def test_onehot_inputs_are_one_hot():
    """the reference's out is the chosen V row, dv the scatter-sum of dO, lse2 the chosen score; every listed position is chosen"""
    B, H, Nq, Nk, causal, q_pos0, _ = _shape(330, 333, 1, 3)
    q, k, v, do, choice = T.onehot_inputs(B, H, Nq, Nk, causal, q_pos0, 5, BF16)
    assert {0, 63, 64, 127, 128, Nk - 1} <= set(choice.tolist()) and Nq - 1 + q_pos0 == Nk - 1 and int((choice == torch.arange(Nq) + q_pos0).sum()) >= Nq // 7
    out, lse2, _, _, dv = T.attn(q, k, v, do, T.FLASH_SCALE, causal, q_pos0)
    scatter = torch.zeros_like(dv).index_add_(2, choice, do.double())
    assert float(scatter.abs().max()) <= 256          # integers a bf16 holds exactly
    # float64 keeps the other keys' 2^-160: equal to 1e-40, and exactly equal once P has passed through fp32
    assert float((out - v.double()[:, :, choice]).abs().max()) <= 1e-40 and float((dv - scatter).abs().max()) <= 1e-40
    ev = T.attn(q, k, v, do, T.FLASH_SCALE, causal, q_pos0, r16=BF16)
    assert torch.equal(ev[0].double(), v.double()[:, :, choice]) and torch.equal(ev[4].double(), scatter)
    score = ((q.double() * T._sl2(T.FLASH_SCALE, True)) * k.double()[:, :, choice]).sum(-1)
    _same(lse2, score, 1e-13)


def test_unseen_keys_and_workspace_formula():
    assert T.unseen_keys(70, 133, 1, 10).nonzero().flatten().tolist() == list(range(80, 133))
    assert T.unseen_keys(70, 200, 1, 0).nonzero().flatten().tolist() == list(range(70, 200))
    assert not bool(T.unseen_keys(70, 133, 1, 63).any()) and not bool(T.unseen_keys(130, 70, 0, 0).any())
    assert T.bwd_workspace_elems(1, 3, 129) == 388 + 3 * 128 * 192 and T.bwd_workspace_elems(1, 1, 64) == 64 + 128 * 64
    for B, H, Nq in ((1, 3, 129), (2, 8, 131), (1, 1, 1)):
        assert T.bwd_workspace_elems(B, H, Nq) <= B * H * (Nq + 3 + 128 * (-(-Nq // 64) * 64))
