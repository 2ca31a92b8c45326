"""tests/train_edge_ref.py on its own, without a GPU: every restatement against torch's float64 op or float64 autograd, every
deliberately wrong restatement outside the bound that tests/test_train_edge_kernels_gpu.py uses at the same inputs, and the plain
fp32 evaluation of each formula inside it."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_ref as E   # noqa: E402
import train_edge_ref as R   # noqa: E402

F32, F64, BF16, F16 = R.F32, R.F64, R.BF16, R.F16


def _same(a, b, tol=1e-12):
    a, b = a.double(), b.double()
    assert (a - b).abs().max().item() <= tol * (b.abs().max().item() + 1e-30), (a - b).abs().max().item()


def _misses(wrong, ref, bnd, what):
    r = R.ratio(wrong, ref, bnd)
    print(f"{what}: wrong / bound = {r:.3g}")
    assert r > 1.0, f"{what}: the wrong variant is inside the bound ({r:.3g})"


def _inside(fn, *args, dtypes=(F32,), **kw):
    """the fp32 evaluation of fn, its outputs rounded to their storage types, is inside the bound"""
    exp = R.expect(fn, *args, dtypes=dtypes, **{k: v for k, v in kw.items()})
    ev = fn(*args, dt=F32, **{k: v for k, v in kw.items() if k not in ("rowwise", "scales")})
    ev = ev if isinstance(ev, tuple) else (ev,)
    for (ref, bnd), e, d in zip(exp, ev, dtypes):
        assert R.ratio(e.to(d), ref, bnd) <= 1.0


# ------------------------------------------------------------------------------------------------------ against torch
def test_activations_match_torch_and_autograd():
    x = R.edge_values(257, 1, F32)
    _same(R.act_fwd(x, R.ACT_GELU), F.gelu(x.double()))
    _same(R.act_fwd(x, R.ACT_SILU), F.silu(x.double()))
    _same(R.act_fwd(x, R.ACT_RELU), F.relu(x.double()))
    _same(R.act_fwd(x, R.ACT_QUICK_GELU), x.double() * torch.sigmoid(1.702 * x.double()))
    assert torch.equal(R.act_fwd(x, 7), x.double())
    dy = R.rand((257,), 2)
    for act in R.ACTS:
        nz = x != 0 if act == R.ACT_RELU else torch.ones_like(x, dtype=torch.bool)      # ReLU'(0) = 0 is the kernel's choice
        _same(R.act_bwd(x, dy, act)[nz], R.autograd_of(lambda v: R.act_fwd(v, act), x, dy)[nz], 1e-9)
        _inside(R.act_fwd, x, act)
        _inside(R.act_bwd, x, dy, act)
    assert bool((R.act_grad(torch.tensor([0.0, -0.0]), R.ACT_RELU) == 0).all())


def test_swiglu_matches_autograd_and_the_swap_shows():
    for dtype in R.DTYPES:
        gu, dy = R.swiglu_inputs(3, 48, 5, dtype)
        g = gu.double().view(3, 3, 2, 16)
        _same(R.swiglu_fwd(gu), (F.silu(g[:, :, 0]) * g[:, :, 1]).reshape(3, 48))
        _same(R.swiglu_bwd(gu, dy), R.autograd_of(R.swiglu_fwd, gu, dy), 1e-9)
        assert bool(torch.isfinite(R.swiglu_fwd(gu, dt=F32)).all()) and bool(torch.isfinite(R.swiglu_bwd(gu, dy, dt=F32)).all())
        (ref, bnd), = R.expect(R.swiglu_fwd, gu, dtypes=(dtype,))
        _misses(R.swiglu_fwd(gu, swapped=True), ref, bnd, f"swiglu fwd swapped {R.IDS[dtype]}")
        (ref, bnd), = R.expect(R.swiglu_bwd, gu, dy, dtypes=(dtype,))
        _misses(R.swiglu_bwd(gu, dy, swapped=True), ref, bnd, f"swiglu bwd swapped {R.IDS[dtype]}")
        _inside(R.swiglu_fwd, gu, dtypes=(dtype,))
        _inside(R.swiglu_bwd, gu, dy, dtypes=(dtype,))


@pytest.mark.parametrize("rms", [0, 1])
def test_norm_adjoint_matches_autograd_and_a_wrong_mean_term_shows(rms):
    eps = R.EPS_RMS if rms else R.EPS_LN
    for dtype in R.DTYPES:
        for rows, C in R.NORM_GENERIC[1:] + R.NORM_VEC[1:]:
            x, dy, w, add = R.norm_inputs(rows, C, C, dtype)
            dx, dyx = R.norm_bwd(x, dy, w, rms, eps)
            _same(dx, R.autograd_of(lambda v: R.norm_fwd(v, w.double(), rms, eps), x, dy), 1e-7)
            if not rms:     # dw = colsum(dy * xhat)
                wv = w.double().clone().requires_grad_(True)
                F.layer_norm(x.double(), (C,), wv, None, eps).backward(dy.double())
                _same(dyx.sum(0), wv.grad, 1e-9)
            (ref, bnd), _ = R.expect(R.norm_bwd, x, dy, w, rms, eps, dtypes=(dtype, F32), rowwise=True)
            flag = {"rms_with_mean_g": True} if rms else {"ln_without_mean_g": True}
            wrong = R.norm_bwd(x, dy, w, rms, eps, **flag)[0]
            _misses(wrong[1:], ref[1:], bnd[1:], f"norm rms={rms} {rows}x{C} {R.IDS[dtype]} mean(g) term")
            _inside(R.norm_bwd, x, dy, w, rms, eps, dtypes=(dtype, F32), rowwise=True)
    x, dy, w, _ = R.norm_inputs(2, 63, 1, F32)
    dx, dyx = R.norm_bwd(x, dy, w, rms, eps)
    if not rms:
        assert bool((dyx[0] == 0).all())          # the constant row: xhat = 0 exactly


def test_softmax_matches_torch_and_a_key_off_shows():
    Nq, rows, sc = R.SOFTMAX_NQ, R.SOFTMAX_ROWS, R.SOFTMAX_SCALE
    for Nk in R.SOFTMAX_NK:
        for causal, p0 in R.softmax_modes(Nk):
            lim = R.softmax_lim(rows, Nq, Nk, causal, p0)
            s = R.softmax_scores(rows, Nk, Nk + 3, lim, Nk)
            ref = R.softmax_fwd(s, Nk, Nk + 2, lim, sc)
            assert bool(torch.isfinite(ref).all()) and bool((ref[:, Nk:] == 0).all())
            z = torch.nan_to_num(s[:, :Nk].double()) * sc
            z = z.masked_fill(torch.arange(Nk)[None, :] >= lim[:, None], -R.INF)
            live = lim > 0
            _same(ref[live, :Nk], torch.softmax(z[live], -1))
            assert bool((ref[~live] == 0).all())
            for dtype in R.DTYPES:
                (r, bnd), = R.expect(R.softmax_fwd, s, Nk, Nk + 2, lim, sc, dtypes=(dtype,))
                _inside(R.softmax_fwd, s, Nk, Nk + 2, lim, sc, dtypes=(dtype,))
                clean = torch.nan_to_num(s, nan=0.3)
                wrongs = [("row // Nq", R.softmax_lim(rows, Nq, Nk, causal, p0, div=True))] if causal else []
                if causal:
                    wrongs += [("limit + 1", R.softmax_lim(rows, Nq, Nk, causal, p0, lim_off=1)), ("limit - 1", R.softmax_lim(rows, Nq, Nk, causal, p0, lim_off=-1))]
                for what, wl in wrongs:
                    if torch.equal(wl, lim):
                        continue        # the mask is saturated at Nk: the mistake cannot show at this geometry
                    _misses(R.softmax_fwd(clean, Nk, Nk + 2, wl, sc), R.softmax_fwd(clean, Nk, Nk + 2, lim, sc), bnd, f"softmax Nk={Nk} p0={p0} {what} {R.IDS[dtype]}")
    # the adjoint against autograd (P unrounded)
    Nk = 65
    lim = R.softmax_lim(rows, Nq, Nk, 1, 3)
    s = torch.nan_to_num(R.softmax_scores(rows, Nk, Nk, lim, 2), nan=-1e9)
    dp = R.rand((rows, Nk), 3)
    p = R.softmax_fwd(s, Nk, Nk, lim, sc)
    auto = R.autograd_of(lambda v: torch.softmax((v * sc).masked_fill(torch.arange(Nk)[None, :] >= lim[:, None], -R.INF), -1), s, dp)
    _same(R.softmax_bwd(p, dp, Nk, Nk, sc), auto, 1e-9)
    _inside(R.softmax_bwd, p, dp, Nk, Nk, sc)


def test_rope_is_a_rotation_and_the_offset_and_sign_show():
    for d in R.ROPE_D:
        for pos0 in R.ROPE_POS0:
            cs = R.rope_table(pos0 + R.ROPE_T, d)
            for dtype in R.DTYPES:
                x = R.rand((R.ROPE_ROWS, R.ROPE_H * d), d + pos0).to(dtype)
                y = R.rope(x, cs, R.ROPE_T, R.ROPE_H, d, pos0, 0)
                # the same rotation as the inference reference, written independently in edge_ref
                q, _, _ = E.rope_cache(torch.cat([x.float(), x.float(), x.float()], 1)[:, :R.ROPE_H * d * 3], cs, 3, R.ROPE_T, R.ROPE_H, R.ROPE_H, d, [pos0] * 3)
                _same(y, q.reshape(R.ROPE_ROWS, -1))
                _same(R.rope(y, cs, R.ROPE_T, R.ROPE_H, d, pos0, 1), x.double(), 4 * R.U32)     # cos^2 + sin^2 of the fp32 table
                g = R.rand(x.shape, 9)
                _same(R.rope(g, cs, R.ROPE_T, R.ROPE_H, d, pos0, 1), R.autograd_of(lambda v: R.rope(v, cs, R.ROPE_T, R.ROPE_H, d, pos0, 0), x, g), 1e-9)
                for adj in (0, 1):
                    (ref, bnd), = R.expect(R.rope, x, cs, R.ROPE_T, R.ROPE_H, d, pos0, adj, dtypes=(dtype,))
                    _inside(R.rope, x, cs, R.ROPE_T, R.ROPE_H, d, pos0, adj, dtypes=(dtype,))
                    if pos0:
                        _misses(R.rope(x, cs, R.ROPE_T, R.ROPE_H, d, pos0, adj, drop_pos0=True), ref, bnd, f"rope d={d} pos0 dropped {R.IDS[dtype]}")
                (ref, bnd), = R.expect(R.rope, x, cs, R.ROPE_T, R.ROPE_H, d, pos0, 1, dtypes=(dtype,))
                _misses(R.rope(x, cs, R.ROPE_T, R.ROPE_H, d, pos0, 1, keep_sign=True), ref, bnd, f"rope d={d} pos0={pos0} sign kept {R.IDS[dtype]}")


def test_cross_entropy_matches_torch_and_a_shifted_label_shows():
    for V in R.CE_V:
        for dtype in R.DTYPES:
            x, labels = R.ce_inputs(V, V, dtype)
            n_valid = int((labels >= 0).sum())
            loss, d = R.cross_entropy(x, labels, 1.0 / n_valid)
            xx = x.double().clone().requires_grad_(True)
            ref = F.cross_entropy(xx, labels, ignore_index=-100)
            ref.backward()
            _same(loss.sum() / n_valid, ref.detach(), 1e-9)
            assert (d - xx.grad).abs().max().item() <= 1e-7          # gscale arrives as fp32(1 / n_valid)
            assert bool((loss[2] == 0)) and bool((d[2] == 0).all())
            sl, sd = R.ce_scales(x, R.CE_GSCALE)
            (rl, bl), (rd, bd) = R.expect(R.cross_entropy, x, labels, R.CE_GSCALE, dtypes=(F32, dtype), scales=(sl, sd))
            _inside(R.cross_entropy, x, labels, R.CE_GSCALE, dtypes=(F32, dtype), scales=(sl, sd))
            if V > 1:
                wl, wd = R.cross_entropy(x, labels, R.CE_GSCALE, onehot_shift=1)
                _misses(wd, rd, bd, f"CE V={V} {R.IDS[dtype]} one-hot at label + 1")
    for dtype in R.DTYPES:
        x, labels = R.ce_extreme(dtype)
        loss, d = R.cross_entropy(x, labels, 1.0)
        _same(loss[0], F.cross_entropy(x.double()[:1], labels[:1]), 1e-9)
        assert bool(torch.isfinite(R.cross_entropy(x, labels, 1.0, dt=F32)[1]).all())


def test_mask_losses_match_torch_and_the_wrong_constants_show():
    for n in R.MASK_N:
        x, t = R.mask_inputs(n, n)
        for wgt in R.MASK_WGT:
            terms = R.mask_terms(x, t, wgt)
            stats = terms.sum(1)
            bce, dice = R.mask_losses(stats, n)
            z = x.double() * wgt
            _same(bce, F.binary_cross_entropy_with_logits(z, t.double(), reduction="none").mean(1), 1e-9)
            p = torch.sigmoid(z)
            _same(dice, 1 - (2 * (p / 1000 * t.double()).sum(1) + 1e-6) / ((p / 1000).sum(1) + (t.double() / 1000).sum(1) + 1e-6), 1e-9)
            ev = R.seq_sum32(R.mask_terms(x, t, wgt, dt=F32), 1)
            assert R.ratio(ev, stats, R.sum_bound(terms, ev, stats, 1)) <= 1.0
            cb, cd = torch.tensor([2.0, 0.5, 1.0]), torch.tensor([0.5, 1.5, 0.25])
            s32 = stats.float()
            _same(R.mask_grad(x, t, stats, wgt, cb, cd), R.mask_grad_autograd(x, t, wgt, cb, cd), 1e-7)
            (ref, bnd), = R.expect(R.mask_grad, x, t, s32, wgt, cb, cd, rowwise=True)
            _inside(R.mask_grad, x, t, s32, wgt, cb, cd, rowwise=True)
            if wgt:
                _misses(R.mask_grad(x, t, s32, wgt, cb, cd, wrong_n=n + 1), ref, bnd, f"mask grad n={n} w={wgt} mean over n + 1")
            if wgt and n == 1:      # the / 1000 only moves the weight of the 1e-6: it shows where the sums are of order 1
                _misses(R.mask_grad(x, t, s32, wgt, cb, cd, no_1000=True), ref, bnd, f"mask grad n={n} w={wgt} dice without / 1000")
                dice32 = torch.stack(R.mask_losses(s32, n), 1)
                _misses(torch.stack(R.mask_losses(stats, n, no_1000=True), 1), torch.stack(R.mask_losses(stats, n), 1), R.bound(torch.stack(R.mask_losses(stats, n), 1), dice32),
                        f"dice n={n} w={wgt} without / 1000")


def test_taxonomy_matches_autograd():
    for C in R.TAX_C:
        for rows in R.TAX_ROWS:
            for soft in (False, True):
                z, t = R.taxonomy_inputs(rows, C, rows + C, soft)
                p, loss, dz = R.taxonomy_ce(z, t)
                _same(p, torch.softmax(z.double(), -1))
                _same(loss, R.taxonomy_loss(z, t), 1e-9)
                assert (dz - R.autograd_of(lambda v: R.taxonomy_loss(v, t), z, torch.ones(rows))).abs().max().item() <= 1e-12
                _inside(R.taxonomy_ce, z, t, dtypes=(F32, F32, F32))


@pytest.mark.parametrize("case", E.RESIZE_CASES, ids=lambda c: f"{c[1]}-{c[2]}-{c[3]}")
def test_bilinear_adjoint_matches_autograd_and_the_two_mistakes_show(case):
    n, src, crop, out = case
    g = R.rand((n, *out), 5)
    ref = R.resize_bwd(g, src, crop)
    _same(ref, R.resize_bwd_autograd(g, src, crop), 1e-9)
    assert bool((ref[:, crop[0]:] == 0).all()) and bool((ref[:, :, crop[1]:] == 0).all())
    (r, bnd), = R.expect(R.resize_bwd, g, src, crop)
    _inside(R.resize_bwd, g, src, crop)
    over = ((R.resize_bwd(g, src, crop, dt=F32).double() - r).abs() > bnd).double().mean().item()
    assert over <= 1e-3          # the exclusion cap of the GPU test; the fp32 scatter needs no exclusion at all
    if any(c > 1 and o > 1 and c != o for c, o in zip(crop, out)):
        _misses(R.resize_bwd(g, src, crop, half_pixel=False), r, bnd, f"bilinear adjoint {case} without the half pixel")
    if crop != src and (crop[0] > 1 or crop[1] > 1):
        wrong = R.resize_bwd(g, src, crop, clamp_to_crop=False)
        if not torch.equal(wrong, r):
            _misses(wrong, r, bnd, f"bilinear adjoint {case} clamped to the source")
    if out[0] * 2 < crop[0]:
        assert bool((ref[:, :crop[0], :crop[1]] == 0).any()), "down-scaling by more than 2 leaves source pixels without gradient"


def test_the_source_clamp_shows_somewhere():
    shown = 0
    for n, src, crop, out in E.RESIZE_CASES:
        g = R.rand((n, *out), 5)
        shown += not torch.equal(R.resize_bwd(g, src, crop, clamp_to_crop=False), R.resize_bwd(g, src, crop))
    assert shown >= 2


def test_scatter_and_sums():
    for name, ids in R.scatter_ids().items():
        dx, dE0 = R.rand((len(ids), 5), 1), R.rand((R.SCATTER_V, 5), 2)
        ref = R.scatter_add(ids, dx, dE0)
        loop = dE0.double().clone()
        for r, i in enumerate(ids.tolist()):
            if i >= 0:
                loop[i] += dx[r].double()
        _same(ref, loop)
    x = R.rand((4099, 8), 3) + 0.3
    ref = x.double().sum(0)
    ev = R.seq_sum32(x)
    bnd = R.sum_bound(x, ev, ref)
    assert R.ratio(ev, ref, bnd) <= 1.0
    _misses(x[:-1].double().sum(0), ref, bnd, "colsum without the last row")


def test_adamw_matches_torch_and_the_wrong_orders_show():
    for wd in (0.0, 0.1):
        for b1, b2 in ((0.9, 0.95), (0.9, 0.999)):
            w, m, v, g = R.adamw_inputs(257, 3, F32)
            p = torch.nn.Parameter(w.double().clone())
            opt = torch.optim.AdamW([p], lr=R.f32(R.ADAMW_LR), betas=(R.f32(b1), R.f32(b2)), eps=R.f32(R.ADAMW_EPS), weight_decay=R.f32(wd))
            mine = (w.double(), torch.zeros(257, dtype=F64), torch.zeros(257, dtype=F64))
            for step in (1, 2, 3):
                gs = R.rand((257,), 10 + step)
                p.grad = gs.double()
                opt.step()
                mine = R.adamw(*mine, gs, R.ADAMW_LR, b1, b2, R.ADAMW_EPS, wd, step, 1.0)
                _same(mine[0], p.detach(), 1e-12)
            # a late step from given moments
            p = torch.nn.Parameter(w.double().clone())
            opt = torch.optim.AdamW([p], lr=R.f32(R.ADAMW_LR), betas=(R.f32(b1), R.f32(b2)), eps=R.f32(R.ADAMW_EPS), weight_decay=R.f32(wd))
            opt.state[p] = {"step": torch.tensor(999.0), "exp_avg": m.double().clone(), "exp_avg_sq": v.double().clone()}
            p.grad = g.double()
            opt.step()
            ref = R.adamw(w, m, v, g, R.ADAMW_LR, b1, b2, R.ADAMW_EPS, wd, 1000, 1.0)
            _same(ref[0], p.detach(), 1e-12)
            _same(ref[1], opt.state[p]["exp_avg"], 1e-12)
            _same(ref[2], opt.state[p]["exp_avg_sq"], 1e-12)
            for step in (1, 2, 1000):
                exp = R.expect(R.adamw, w, m, v, g, R.ADAMW_LR, b1, b2, R.ADAMW_EPS, wd, step, 0.5, dtypes=(F32, F32, F32))
                _inside(R.adamw, w, m, v, g, R.ADAMW_LR, b1, b2, R.ADAMW_EPS, wd, step, 0.5, dtypes=(F32, F32, F32))
                if step == 2 or (step == 1000 and b2 == 0.999):     # 1 - 0.95^1000 is 1 in every format: nothing can show there
                    _misses(R.adamw(w, m, v, g, R.ADAMW_LR, b1, b2, R.ADAMW_EPS, wd, step, 0.5, bc_step_off=-1)[0], *exp[0], f"AdamW step {step} b2 {b2} bias correction with step - 1")
                if wd:
                    _misses(R.adamw(w, m, v, g, R.ADAMW_LR, b1, b2, R.ADAMW_EPS, wd, step, 0.5, decay_after=True)[0], *exp[0], f"AdamW step {step} decay after the update")
    w, m, v, g = R.adamw_inputs(257, 3, F32)
    out = R.adamw(w, m, v, g, R.ADAMW_LR, 0.9, 0.95, R.ADAMW_EPS, 0.1, 1, 1.0)
    assert torch.equal(out[0][::97], w.double()[::97] - R.f32(R.ADAMW_LR) * R.f32(0.1) * w.double()[::97])


def test_half_ulp_is_the_storage_rounding():
    x = R.rand((4096,), 1, 3.0).double()
    for dtype in (BF16, F16):
        assert bool(((x.to(dtype).double() - x).abs() <= R.half_ulp(x, dtype)).all())
        assert bool(((x.to(dtype).double() - x).abs() > 0.25 * R.half_ulp(x, dtype)).any())
