"""All-projection LoRA and fp16 fine-tuning at the shapes the fine-tune step runs (Llama 7B: H 4096 / 32 heads / F 11008, 13B:
5120 / 40 / 13824; M = 351 = one 351-token sample and 2808 = the bench batch of 8): haff_lora_out, haff_lora_gu_swiglu and haff_lora_tn
through the C ABI against fp64 (past the 8192-block grid cap, with pad columns, in both 16-bit types); the fused adapter nodes
against torch fp32 autograd of their definition, against the generic composition and against themselves; the all-seven and the
q,v trainers at 7B width against the oracle in bf16 and fp16; and ranks off the fused path (r > 8: the generic composition; r < 8:
the padded fused nodes, and the generic composition with a padded rank) at the mid geometry."""
import os
import sys
import time

import pytest
import torch

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from test_lora_targets_gpu import ALL7, MID_CLASS_TOL, _close, _interleave, _merged_oracle, _rope_ref  # noqa: E402

DTYPES = [torch.bfloat16, torch.float16]
GEOMS = {"7b": (4096, 32, 11008), "13b": (5120, 40, 13824)}   # hidden, heads, ffn
T = 351                                                         # tokens per sample: M = 351 is one sample, 2808 eight


def _lib():
    import haff  # noqa: F401
    from haff.lib import load_library
    return load_library()


def _fn(lib, name, dtype):
    return getattr(lib, name + "_f16") if dtype == torch.float16 else getattr(lib, name)


def _rn(shape, g, scale=1.0):
    return torch.randn(shape, generator=g, device=g.device) * scale


def _ulp(ref, dtype):
    """one unit in the last place of the 16-bit type at |ref| (fp64; subnormal spacing below the normal range)"""
    p, emin = (7, -126) if dtype == torch.bfloat16 else (10, -14)
    e = torch.floor(torch.log2(ref.abs().clamp_min(2.0 ** emin)))
    return torch.pow(2.0, e - p)


def _within(got, ref, dtype, n_ulp, slack, what):
    """|got - ref| <= n_ulp ulps of ref + slack (the fp32 arithmetic's own rounding, from the sum of |terms|)"""
    got = got.double()
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs()
    ulps = (err / _ulp(ref, dtype)).max().item()
    worst = (err / (n_ulp * _ulp(ref, dtype) + slack)).max().item()
    print(f"{what}: max {ulps:.3f} ulps, err / bound {worst:.3f}")
    assert worst <= 1.0, (what, ulps, worst)


def _s32(v):
    return float(torch.tensor(v, dtype=torch.float32))


# ---- 1. the kernels through the C ABI, against fp64 -----------------------------------------------------------------------------
def _rank_rows_with_pads(R, M, g, dtype, pad_value=3.0):
    """t^T [R][roundup(M, 16)]: random ranks, the pad columns finite and non-zero (they must not reach any result)"""
    ldt = (M + 15) // 16 * 16
    t = torch.full((R, ldt), pad_value, device=g.device)
    t[:, :M] = _rn((R, M), g)
    return t.to(dtype), ldt


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("N", [4096, 5120])
@pytest.mark.parametrize("M", [1, 3, 351, 2808, 16421])
def test_lora_out_kernel_fp64(dev, dtype, N, M):
    """haff_lora_out: y[m] += s t[m] B^T on the rows m < M of a wider, taller y, within one ulp of the fp64 result rounded once.
    M = 16421 (not a multiple of 4) has (M + 3) / 4 * N / 8 > 8192 * 256 work items: the grid-stride loop's second pass runs."""
    lib = _lib()
    g = torch.Generator(device=dev).manual_seed(100 + M + N)
    s = _s32(2.0 / 0.7)
    tT, ldt = _rank_rows_with_pads(8, M, g, dtype)
    B = _rn((N, 8), g, 0.3).to(dtype)
    ldy = N + 16
    y = _rn((M + 5, ldy), g).to(dtype)
    y0 = y.clone()
    assert _fn(lib, "haff_lora_out", dtype)(tT.data_ptr(), ldt, B.data_ptr(), y.data_ptr(), ldy, M, N, s, None) == 0
    torch.cuda.synchronize()
    t64, b64 = tT[:, :M].double(), B.double()
    ref = y0[:M, :N].double() + s * (t64.t() @ b64.t())
    mag = y0[:M, :N].double().abs() + s * (t64.abs().t() @ b64.abs().t())
    _within(y[:M, :N], ref, dtype, 1, 2.0 ** -21 * mag, f"lora_out {dtype} M{M} N{N}")
    assert torch.equal(y[M:], y0[M:]) and torch.equal(y[:, N:], y0[:, N:])   # rows past M and columns past N untouched


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("F", [11008, 13824])
@pytest.mark.parametrize("M,which", [(2808, "both"), (6203, "both"), (2808, "up_only")])
def test_lora_gu_swiglu_kernel_fp64(dev, dtype, F, M, which):
    """haff_lora_gu_swiglu: gu' = gu + s [tg Bg^T | tu Bu^T] in the interleaved [gate x16 | up x16] layout (in place, within one
    ulp of fp64), y = silu(g') u' of the STORED g', u' (within two ulps). M = 6203 passes the grid cap at F = 11008 and 13824.
    up_only: the gate adapter's rank rows are zero, so an update landing on the wrong half of a group fails."""
    lib = _lib()
    g = torch.Generator(device=dev).manual_seed(200 + M + F)
    s = _s32(16.0 / 8 / 0.95)
    tT, ldt = _rank_rows_with_pads(16, M, g, dtype)
    if which == "up_only":
        tT[0:8] = 0
    Bg, Bu = _rn((F, 8), g, 0.3).to(dtype), _rn((F, 8), g, 0.3).to(dtype)
    gu = _rn((M + 3, 2 * F), g).to(dtype)
    y = _rn((M + 3, F), g).to(dtype)
    gu0, y0 = gu.clone(), y.clone()
    assert _fn(lib, "haff_lora_gu_swiglu", dtype)(tT.data_ptr(), ldt, Bg.data_ptr(), Bu.data_ptr(), gu.data_ptr(), 2 * F, y.data_ptr(), F,
                                                 M, F, s, None) == 0
    torch.cuda.synchronize()
    tg, tu = tT[0:8, :M].double(), tT[8:16, :M].double()
    upd = _interleave(tg.t() @ Bg.double().t(), tu.t() @ Bu.double().t())
    mag = gu0[:M].double().abs() + s * _interleave(tg.abs().t() @ Bg.double().abs().t(), tu.abs().t() @ Bu.double().abs().t())
    ref = gu0[:M].double() + s * upd
    if which == "up_only":
        gate_cols = ref.view(M, F // 16, 2, 16)[:, :, 0]
        assert torch.equal(gate_cols, gu0[:M].double().view(M, F // 16, 2, 16)[:, :, 0])
    _within(gu[:M], ref, dtype, 1, 2.0 ** -21 * mag, f"lora_gu_swiglu gu' {dtype} M{M} F{F} {which}")
    stored = gu[:M].double().view(M, F // 16, 2, 16)
    gs, us = stored[:, :, 0].reshape(M, F), stored[:, :, 1].reshape(M, F)
    _within(y[:M], torch.nn.functional.silu(gs) * us, dtype, 2, 0.0, f"lora_gu_swiglu y {dtype} M{M} F{F} {which}")
    assert torch.equal(gu[M:], gu0[M:]) and torch.equal(y[M:], y0[M:])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("R,N", [(8, 4096), (8, 11008), (8, 13824), (16, 22016), (16, 27648)])
@pytest.mark.parametrize("M", [351, 2808, 22464])
def test_lora_tn_kernel_fp64(dev, dtype, R, N, M):
    """haff_lora_tn: out = s sT[:, :M] big (the contraction over rows: per-row-block partials summed in index order) against fp64,
    within 1e-6 of the sum of |terms| (f32 out) and one ulp more (16-bit out), in the plain [j][n] and the transposed [n][j]
    layouts, all R rank rows or j_valid < R of them; a second launch gives the same bits. 22464 rows: the batch of 64."""
    lib = _lib()
    g = torch.Generator(device=dev).manual_seed(300 + M + N + R)
    s = _s32(2.0 / 0.7)
    sT, lds = _rank_rows_with_pads(R, M, g, dtype)
    ldb = N + 64
    big = _rn((M, ldb), g).to(dtype)
    big[:, N:] = 5.0
    ref = torch.empty((R, N), dtype=torch.float64, device=dev)
    mag = torch.empty((R, N), dtype=torch.float64, device=dev)
    s64 = sT[:, :M].double()
    for c in range(0, N, 4096):   # fp64 in column slabs: the whole big operand in fp64 is 5 GB at M = 22464
        e = min(c + 4096, N)
        b64 = big[:, c:e].double()
        ref[:, c:e] = s * (s64 @ b64)
        mag[:, c:e] = abs(s) * (s64.abs() @ b64.abs())
        del b64
    n_ws = lib.haff_lora_tn_workspace_elems(M, R, N)
    assert n_ws > 0
    ws = torch.empty((n_ws,), dtype=torch.float32, device=dev)
    fn = _fn(lib, "haff_lora_tn", dtype)
    for transposed, j_valid, out_f32 in ((0, R, 0), (1, R - 3, 0), (0, R, 1), (1, R, 1)):
        odt = torch.float32 if out_f32 else dtype
        shape = (N, j_valid + 2) if transposed else (R, N + 8)
        out = torch.full(shape, 7.0, dtype=odt, device=dev)
        ldo = out.stride(0)
        outs = []
        for _ in range(2):
            out.fill_(7.0)
            assert fn(sT.data_ptr(), lds, R, big.data_ptr(), ldb, M, N, ws.data_ptr(), ws.numel(), out.data_ptr(), ldo, out_f32,
                      transposed, j_valid, s, None) == 0
            torch.cuda.synchronize()
            outs.append(out.clone())
        assert torch.equal(outs[0], outs[1]), "second launch differs"
        got = out[:, :j_valid].t() if transposed else out[:j_valid, :N]
        what = f"lora_tn {dtype} R{R} N{N} M{M} {'[n][j]' if transposed else '[j][n]'} j_valid {j_valid} {'f32' if out_f32 else '16-bit'}"
        if out_f32:
            err = ((got.double() - ref[:j_valid]).abs() / mag[:j_valid]).max().item()
            print(f"{what}: max err / sum|terms| {err:.3e}")
            assert err <= 1e-6, (what, err)
        else:
            _within(got, ref[:j_valid], dtype, 1, 1e-6 * mag[:j_valid], what)
        rest = out[:, j_valid:] if transposed else torch.cat([out[j_valid:].reshape(-1), out[:, N:].reshape(-1)])
        assert (rest == 7.0).all(), what   # nothing written past j_valid / N


# ---- 2. the fused adapter nodes at production geometry ------------------------------------------------------------------------
def _node_tol(dtype, gate_up=False):
    if gate_up:
        return 3e-2 if dtype == torch.bfloat16 else 5e-3
    return 2e-2 if dtype == torch.bfloat16 else 4e-3


class _NoTF32:
    def __enter__(self):
        self.saved = torch.backends.cuda.matmul.allow_tf32
        torch.backends.cuda.matmul.allow_tf32 = False

    def __exit__(self, *exc):
        torch.backends.cuda.matmul.allow_tf32 = self.saved


def _run(fn, inputs, dys):
    """outputs and input gradients of fn(*leaves) (inputs None stay None) under the cotangents dys"""
    leaves = [None if t is None else t.detach().clone().requires_grad_(True) for t in inputs]
    outs = fn(*leaves)
    torch.autograd.backward(list(outs), [d.to(outs[0].dtype) for d in dys])
    return [o.detach() for o in outs], [None if t is None else t.grad for t in leaves]


def _check_node(what, dtype, tol, fused, generic, ref, inputs, names, dys):
    """fused against torch fp32 of the definition on the same rounded inputs (max error over max |ref| <= tol, every output and
    gradient), no further from it than the generic composition (summed mean errors, 1.25x), and repeatable to the bit."""
    x16 = [None if t is None else t.to(dtype) for t in inputs]
    x32 = [None if t is None else t.float() for t in x16]
    with _NoTF32():
        r_out, r_grad = _run(ref, x32, [d.to(dtype).float() for d in dys])
    f_out, f_grad = _run(fused, x16, dys)
    g_out, g_grad = _run(generic, x16, dys)
    pairs = [(f"y{i}", f, g, r) for i, (f, g, r) in enumerate(zip(f_out, g_out, r_out))]
    pairs += [(f"d{n}", f, g, r) for n, f, g, r in zip(names, f_grad, g_grad, r_grad) if r is not None]
    e_f = e_g = 0.0
    for n, f, g, r in pairs:
        _close(f, r.cpu(), tol, f"{what} {n}")
        scale = r.abs().mean().item() + 1e-30
        e_f += (f.float() - r).abs().mean().item() / scale
        e_g += (g.float() - r).abs().mean().item() / scale
    print(f"{what}: summed mean error fused {e_f:.3e} generic {e_g:.3e}")
    assert e_f <= 1.25 * e_g, (what, e_f, e_g)
    f2_out, f2_grad = _run(fused, x16, dys)
    for a, b in zip(f_out + f_grad, f2_out + f2_grad):
        assert (a is None and b is None) or torch.equal(a, b), f"{what}: second run differs"


# geometry x rows x rank: every combination at ranks 8 and 4, and rank 1 (seven zero rank rows in every padded operand) at one
# shape per geometry
GMR = [(g, m, r) for g in GEOMS for m in (351, 2808) for r in (8, 4)] + [("7b", 351, 1), ("13b", 2808, 1)]


def _dy_scale(r):
    """the cotangent's scale: r / 16, so that s dy (s = 16 / r) and the adapter gradients stay one size at every rank (rank 1's
    at unit scale pass fp16's 65504)"""
    return r / 16.0


def _keep(shape, g, p=0.3):
    return (torch.rand(shape, generator=g, device=g.device) >= p).float()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geom,M,r", GMR)
@pytest.mark.parametrize("proj", ["o_proj", "down_proj"])
@pytest.mark.parametrize("masked", [False, True])
def test_lora_linear_node_fullsize(dev, dtype, geom, proj, M, r, masked):
    """A.lora_linear (frozen product + residual, haff_lora_out; adjoint: two rank products, haff_lora_tn twice, haff_lora_dx)."""
    from haff import autograd as A
    from haff.train_model import DropoutMul, lora_delta
    H, _, F = GEOMS[geom]
    K, N = (H, H) if proj == "o_proj" else (F, H)
    g = torch.Generator(device=dev).manual_seed(400 + M + K + r)
    w = _rn((N, K), g, K ** -0.5).to(dtype)
    wt = A.transpose(w)[0]
    w32 = w.float()
    s = 16.0 / r / (0.7 if masked else 1.0)
    keep = _keep((M, K), g) if masked else None
    k16 = None if keep is None else keep.to(dtype)
    inputs = [_rn((M, K), g), _rn((M, N), g), _rn((r, K), g, K ** -0.5), _rn((N, r), g, 0.2)]

    def fused(x, res, a, b):
        return [A.lora_linear(x, w, wt, res, a, b, s, k16)]

    def generic(x, res, a, b):
        xd = x if k16 is None else DropoutMul.apply(x, k16)
        return [A.add(A.linear(x, w, None, res, wt), lora_delta(xd, a, b, s))]

    def ref(x, res, a, b):
        xd = x if keep is None else x * keep
        return [x @ w32.t() + res + s * (xd @ a.t()) @ b.t()]

    _check_node(f"{proj} {geom} {dtype} M{M} r{r} masked {masked}", dtype, _node_tol(dtype), fused, generic, ref, inputs,
                ["x", "resid", "A", "B"], [_rn((M, N), g, _dy_scale(r))])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geom,M,r", GMR)
@pytest.mark.parametrize("masks", ["none", "shared", "per_adapter"])
def test_lora_gate_up_swiglu_node_fullsize(dev, dtype, geom, M, r, masks):
    """A.lora_gate_up_swiglu (haff_lora_gu_swiglu; adjoint: the 16-row rank product over K = 2F, haff_lora_tn with R = 16 over
    N = 2F, haff_lora_dx / dx2) at F = 11008 / 13824."""
    from haff import autograd as A
    from haff.train_model import DropoutMul, lora_delta
    H, _, F = GEOMS[geom]
    K = H
    g = torch.Generator(device=dev).manual_seed(500 + M + K + r)
    w = _rn((2 * F, K), g, K ** -0.5).to(dtype)
    wt = A.transpose(w)[0]
    w32 = w.float()
    s = 16.0 / r / (1.0 if masks == "none" else 0.7)
    kg = ku = None
    if masks != "none":
        kg = _keep((M, K), g)
        ku = kg if masks == "shared" else _keep((M, K), g)
    k16 = None if kg is None else (kg.to(dtype) if masks == "shared" else (kg.to(dtype), ku.to(dtype)))
    inputs = [_rn((M, K), g), _rn((r, K), g, K ** -0.5), _rn((F, r), g, 0.2), _rn((r, K), g, K ** -0.5), _rn((F, r), g, 0.2)]

    def fused(x, ag, bg, au, bu):
        return [A.lora_gate_up_swiglu(x, w, wt, ag, bg, au, bu, s, k16)]

    def generic(x, ag, bg, au, bu):
        gu = A.linear(x, w, None, None, wt)
        xg = x if kg is None else DropoutMul.apply(x, k16 if masks == "shared" else k16[0])
        xu = x if ku is None else (xg if masks == "shared" else DropoutMul.apply(x, k16[1]))
        dg, du = lora_delta(xg, ag, bg, s), lora_delta(xu, au, bu, s)
        d = torch.cat([dg.view(M, F // 16, 1, 16), du.view(M, F // 16, 1, 16)], dim=2).reshape(M, 2 * F)
        return [A.swiglu(A.add(gu, d))]

    def ref(x, ag, bg, au, bu):
        xg = x if kg is None else x * kg
        xu = x if ku is None else x * ku
        gu = x @ w32.t() + _interleave(s * (xg @ ag.t()) @ bg.t(), s * (xu @ au.t()) @ bu.t())
        v = gu.view(M, F // 16, 2, 16)
        return [torch.nn.functional.silu(v[:, :, 0].reshape(M, F)) * v[:, :, 1].reshape(M, F)]

    _check_node(f"gate|up {geom} {dtype} M{M} r{r} masks {masks}", dtype, _node_tol(dtype, True), fused, generic, ref, inputs,
                ["x", "Ag", "Bg", "Au", "Bu"], [_rn((M, F), g, _dy_scale(r))])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("geom,M,r", GMR)
@pytest.mark.parametrize("case", ["qkv_three", "k_only"])
@pytest.mark.parametrize("masks", ["none", "shared", "per_adapter"])
def test_lora_qkv3_rope_node_fullsize(dev, dtype, geom, M, r, case, masks):
    """A.lora_qkv3_rope (haff_lora_qkv3_rope_fwd with the k adapter; adjoint haff_lora_qkv_rope_bwd, haff_lora_tn, haff_lora_dx3) at
    32 / 40 heads of 128."""
    from haff import autograd as A
    from haff.train_model import DropoutMul, lora_delta
    H, heads, _ = GEOMS[geom]
    g = torch.Generator(device=dev).manual_seed(600 + M + H + r)
    theta = torch.rand((T, 64), generator=g, device=dev) * 6.0
    cs = torch.cat([theta.cos(), theta.sin()], 1).contiguous()
    w = _rn((3 * H, H), g, H ** -0.5).to(dtype)
    wt = A.transpose(w)[0]
    w32 = w.float()
    on = [True, True, True] if case == "qkv_three" else [False, False, True]   # q, v, k
    s = 16.0 / r / (1.0 if masks == "none" else 0.7)
    km = [None] * 3
    if masks != "none":
        km = [_keep((M, H), g)] * 3 if masks == "shared" else [_keep((M, H), g) for _ in range(3)]
    k16 = None if masks == "none" else (km[0].to(dtype) if masks == "shared" else tuple(k.to(dtype) for k in km))
    inputs = [_rn((M, H), g)]
    for i in range(3):
        inputs += [_rn((r, H), g, H ** -0.5), _rn((H, r), g, 0.2)] if on[i] else [None, None]

    def fused(x, aq, bq, av, bv, ak, bk):
        return list(A.lora_qkv3_rope(x, w, wt, aq, bq, av, bv, ak, bk, cs, T, heads, s, k16))

    def generic(x, aq, bq, av, bv, ak, bk):   # the trainer's composition (LisaTrainable._llm without a fused q|k|v node)
        qkv = A.linear(x, w, None, None, wt)
        outs = [qkv[:, :H], qkv[:, 2 * H:], qkv[:, H:2 * H]]
        for i, (a, b) in enumerate(((aq, bq), (av, bv), (ak, bk))):
            if a is not None:
                m16 = None if km[i] is None else (k16 if masks == "shared" else k16[i])
                outs[i] = A.add(outs[i], lora_delta(x if m16 is None else DropoutMul.apply(x, m16), a, b, s))
        q, v, k = outs
        return [A.rope(q, cs, T, heads, 128), A.rope(k, cs, T, heads, 128), v if av is not None else v.contiguous()]

    def ref(x, aq, bq, av, bv, ak, bk):
        qkv = x @ w32.t()
        outs = [qkv[:, :H], qkv[:, 2 * H:], qkv[:, H:2 * H]]
        for i, (a, b) in enumerate(((aq, bq), (av, bv), (ak, bk))):
            if a is not None:
                xd = x if km[i] is None else x * km[i]
                outs[i] = outs[i] + s * (xd @ a.t()) @ b.t()
        return [_rope_ref(outs[0], cs, T), _rope_ref(outs[2], cs, T), outs[1]]

    _check_node(f"q|k|v {geom} {dtype} M{M} r{r} {case} masks {masks}", dtype, _node_tol(dtype), fused, generic, ref, inputs,
                ["x", "Aq", "Bq", "Av", "Bv", "Ak", "Bk"], [_rn((M, H), g, _dy_scale(r)) for _ in range(3)])


# ---- 3. the trainer at 7B width against the oracle ----------------------------------------------------------------------------
def _trainer_vs_oracle(dev, cfg, sd, batch, dtype, targets, lora_r=8):
    """losses, per-class worst relative L2 gradient error and the global gradient cosine of LisaTrainable against the oracle on
    weights with every adapter merged (fp32, CPU autograd)"""
    from test_train_gpu import grad_class
    from haff.train_model import LisaTrainable
    model = LisaTrainable(cfg, sd, dtype=dtype, device=dev, lora_r=lora_r, lora_dropout=0.0, lora_init_b_zero=False, seed=3,
                          lora_target_modules=targets)
    t0 = time.time()
    ref, leaves = _merged_oracle(cfg, sd, model, batch)
    t_oracle = time.time() - t0
    out = model(**{k: (v.to(dev) if torch.is_tensor(v) else v) for k, v in batch.items()})
    out["loss"].backward()
    losses = {k: (float(out[k].detach()), float(ref[k].detach())) for k in ref}
    by_class, fg, fr, worst = {}, [], [], {}
    for k, p in model.named_parameters():
        r = leaves[k].grad
        if r is None or r.abs().max().item() < 1e-6:
            continue
        assert p.grad is not None, k
        rel = ((p.grad.float().cpu() - r).norm() / (r.norm() + 1e-12)).item()
        c = grad_class(k)
        if rel >= by_class.get(c, 0.0):
            by_class[c], worst[c] = rel, k
        fg.append(p.grad.float().cpu().reshape(-1))
        fr.append(r.reshape(-1))
    cos = torch.nn.functional.cosine_similarity(torch.cat(fg).double(), torch.cat(fr).double(), dim=0).item()
    n_lora = sum(1 for k in model.params if "lora_" in k and leaves[k].grad is not None)
    print("worst tensor per class: " + ", ".join(f"{c} {worst[c]}" for c in sorted(worst)))
    return model, losses, by_class, cos, n_lora, t_oracle


def _report_and_check(what, losses, by_class, cos, tol):
    for k, (a, b) in losses.items():
        print(f"{what} {k}: hip {a:.6f} oracle {b:.6f}")
    print(f"{what}: worst per class " + ", ".join(f"{c} {v:.3e}" for c, v in sorted(by_class.items())))
    print(f"{what}: global gradient cosine {cos:.6f}")
    for k, (a, b) in losses.items():
        assert abs(a - b) <= 3e-2 * max(1.0, abs(b)), (what, k, a, b)
    for c, v in by_class.items():
        assert v <= tol.get(c, 0.25), (what, c, v)
    assert cos >= 0.995, (what, cos)


def _cfg_7b_width():
    from haff import config as hcfg
    return hcfg.LisaCfg(name="7B-width, reduced depth", sam=hcfg.SamCfg(depth=2, global_idx=(1,)), clip=hcfg.ClipCfg(layers=2),
                        llm=hcfg.LlamaCfg(layers=1))


# worst per-tensor relative L2 gradient error per class at 7B width (1 Llama layer) against the merged-adapter oracle, measured on
# MI355X; each bound is at most 2x its measurement (classes whose 2x passes 0.25 keep the per-tensor 0.25 of the other tests).
# all seven, bf16: lora_A 1.42e-2, lora_B 1.59e-2, embed_tokens 9.30e-3, lm_head 5.29e-3, text_hidden_fcs 0.103, decoder
# upscaling 1.01e-2, hypernetworks 7.07e-2, taxonomy_embed 0.181, tokens 0.137, transformer 0.158; cosine 0.99948
TOL_7B_ALL7_BF16 = {"lora_A": 2.8e-2, "lora_B": 3.1e-2, "embed_tokens": 1.8e-2, "lm_head": 1.0e-2, "text_hidden_fcs": 0.2,
                    "decoder.output_upscaling": 2e-2, "decoder.output_hypernetworks": 0.14}
# all seven, fp16: lora_A 3.16e-3, lora_B 2.96e-3, embed_tokens 1.49e-3, lm_head 6.51e-4, text_hidden_fcs 1.89e-2, decoder
# upscaling 2.02e-3, hypernetworks 1.69e-3, taxonomy_embed 1.47e-3, tokens 4.25e-2, transformer 2.74e-2; cosine 0.999993
TOL_7B_ALL7_FP16 = {"lora_A": 6.3e-3, "lora_B": 5.9e-3, "embed_tokens": 2.9e-3, "lm_head": 1.3e-3, "text_hidden_fcs": 3.7e-2,
                    "decoder.output_upscaling": 4e-3, "decoder.output_hypernetworks": 3.3e-3, "decoder.taxonomy_embed": 2.9e-3,
                    "decoder.token": 8.5e-2, "decoder.transformer": 5.4e-2}
# q,v, fp16: lora_A 3.28e-3, lora_B 3.64e-3, embed_tokens 2.10e-3, lm_head 5.50e-4, text_hidden_fcs 2.79e-2, decoder upscaling
# 1.97e-3, hypernetworks 1.40e-3, taxonomy_embed 1.41e-3, tokens 4.14e-2, transformer 2.88e-2; cosine 0.999993
TOL_7B_QV_FP16 = {"lora_A": 6.5e-3, "lora_B": 7.2e-3, "embed_tokens": 4.1e-3, "lm_head": 1.1e-3, "text_hidden_fcs": 5.5e-2,
                  "decoder.output_upscaling": 3.9e-3, "decoder.output_hypernetworks": 2.8e-3, "decoder.taxonomy_embed": 2.8e-3,
                  "decoder.token": 8.2e-2, "decoder.transformer": 5.7e-2}


# 13-14 s each on MI355X, the oracle's CPU forward / backward 4-5 s of it
@pytest.mark.timeout(300)
@pytest.mark.parametrize("mode,targets", [("bf16", ALL7), ("fp16", ALL7), ("fp16", "q_proj,v_proj")])
def test_trainer_at_7b_width_matches_oracle(dev, mode, targets):
    """The 7B-width fine-tune step (the geometry of test_configs_gpu.py::test_finetune_forward_backward_at_7b_width) with all seven
    adapters in bf16 and fp16, and the default q,v adapters in fp16, against the oracle with every adapter merged into its weight."""
    import haff  # noqa: F401
    from haff import weights as hw
    from test_fp16_train_gpu import _exact_in_all
    from test_train_gpu import make_batch
    t0 = time.time()
    cfg = _cfg_7b_width()
    sd = hw.make_state_dict(cfg, 21)
    batch = make_batch(cfg, hw=(100, 90))
    if mode == "bf16":
        hw.round_to_bf16_(sd)
        batch["images"] = batch["images"].to(torch.bfloat16).float()
        batch["images_clip"] = batch["images_clip"].to(torch.bfloat16).float()
    else:
        _exact_in_all(sd)
        batch["images"] = _exact_in_all({"x": batch["images"]})["x"]
        batch["images_clip"] = _exact_in_all({"x": batch["images_clip"]})["x"]
    dtype = torch.bfloat16 if mode == "bf16" else torch.float16
    model, losses, by_class, cos, n_lora, t_oracle = _trainer_vs_oracle(dev, cfg, sd, batch, dtype, targets)
    assert n_lora == 2 * len(model.lora_modules) == (14 if targets == ALL7 else 4)
    tol = {("bf16", ALL7): TOL_7B_ALL7_BF16, ("fp16", ALL7): TOL_7B_ALL7_FP16}.get((mode, targets), TOL_7B_QV_FP16)
    what = f"7B width {mode} {'all seven' if targets == ALL7 else 'q,v'}"
    print(f"{what}: {time.time() - t0:.1f} s (oracle {t_oracle:.1f} s)")
    _report_and_check(what, losses, by_class, cos, tol)


# ---- 4. ranks off the fused path (mid geometry) ------------------------------------------------------------------------------
# MID_CLASS_TOL holds at every rank but one class at rank 1 on the fused nodes: the worst lora_A (layer 1 k_proj's) measured 5.91e-2
# on MI355X, where the generic composition measured 2.49e-2 and rank 8 1.75e-2. k's gradient comes through the softmax adjoint (each
# query's score gradients sum to zero): small differences of large terms, which move with every rounding upstream (a 1.5 % change
# of a quarter of the o_proj / down_proj updates brought this one under 3e-2). The rank-1 nodes themselves are pinned against fp32
# at production width above; the bound is 2x the measurement.
RANK1_FUSED_CLASS_TOL = {**MID_CLASS_TOL, "lora_A": 0.12}


@pytest.mark.parametrize("lora_r,fused", [(16, True), (4, True), (1, True), (4, False), (1, False)])
def test_all_seven_ranks_match_oracle(dev, lora_r, fused):
    """All seven targets at the mid geometry in bf16 with ranks other than 8: r = 16 runs the generic composition (the fused nodes
    take rank <= 8), r = 4 and 1 the fused nodes on rank-padded operands, and r = 4 with the fused nodes switched off the generic
    composition on a rank that is not a multiple of 8. Which path ran is counted, not assumed."""
    import haff  # noqa: F401
    from haff import autograd as A
    from haff import config as hcfg, weights as hw
    from test_train_gpu import make_batch
    cfg = hcfg.mid()
    sd = hw.round_to_bf16_(hw.make_state_dict(cfg, 21))
    batch = make_batch(cfg)
    batch["images"] = batch["images"].to(torch.bfloat16).float()
    batch["images_clip"] = batch["images_clip"].to(torch.bfloat16).float()
    calls = {"fused": 0, "supported": [], "qkv_supported": []}
    saved = {n: getattr(A, n) for n in ("lora_linear", "lora_gate_up_swiglu", "lora_qkv3_rope", "lora_fused_supported",
                                         "lora_qkv_rope_supported", "FUSED_LORA_QKV", "FUSED_LORA_OUT", "FUSED_LORA_GATE_UP")}

    def counted(fn):
        def wrapper(*a, **k):
            calls["fused"] += 1
            return fn(*a, **k)
        return wrapper

    def spy(fn, key):
        def wrapper(*a, **k):
            v = fn(*a, **k)
            calls[key].append(v)
            return v
        return wrapper
    try:
        for n in ("lora_linear", "lora_gate_up_swiglu", "lora_qkv3_rope"):
            setattr(A, n, counted(saved[n]))
        A.lora_fused_supported = spy(saved["lora_fused_supported"], "supported")
        A.lora_qkv_rope_supported = spy(saved["lora_qkv_rope_supported"], "qkv_supported")
        if not fused:
            A.FUSED_LORA_QKV = A.FUSED_LORA_OUT = A.FUSED_LORA_GATE_UP = False
        model, losses, by_class, cos, n_lora, _ = _trainer_vs_oracle(dev, cfg, sd, batch, torch.bfloat16, ALL7, lora_r=lora_r)
    finally:
        for n, v in saved.items():
            setattr(A, n, v)
    L = cfg.llm.layers
    assert n_lora == 14 * L
    assert model.params["model.layers.0.self_attn.q_proj.lora_A"].shape[0] == lora_r
    if fused and lora_r <= 8:
        assert calls["fused"] == 4 * L, calls   # q|k|v, o_proj, gate|up, down_proj: every layer
        assert all(calls["supported"]) and all(calls["qkv_supported"]), calls
    elif fused:
        assert calls["fused"] == 0 and calls["supported"] and not any(calls["supported"]), calls
        assert calls["qkv_supported"] and not any(calls["qkv_supported"]), calls
    else:
        assert calls["fused"] == 0 and not calls["supported"] and not calls["qkv_supported"], calls
    tol = RANK1_FUSED_CLASS_TOL if (lora_r, fused) == (1, True) else MID_CLASS_TOL
    _report_and_check(f"mid bf16 all seven r{lora_r} {'fused' if fused else 'generic'}", losses, by_class, cos, tol)
