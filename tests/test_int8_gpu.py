"""The LLM.int8 8-bit mode on the MI355X: the device weight and activation quantisers and the int8 product bit for bit against the
independent CPU restatement (tests/int8_ref.py) at the 7B / 13B / lm_head shapes, both product forms and every M giving one row the
same bits, the residual / SwiGLU epilogues, and LisaMI355(load_in_8bit=True) against the oracle whose converted Linears run int8_ref
one frame per call (the reference's own call pattern, use_cache=False)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/int8_ref.py
import int8_ref as R   # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES_7B = {"qkv": (3 * 4096, 4096), "o": (4096, 4096), "gate_up": (2 * 11008, 4096), "down": (4096, 11008), "lm_head": (32001, 4096)}
SHAPES_13B = {"qkv": (3 * 5120, 5120), "down": (5120, 13824)}


def _rows(M, K, seed, planted=(), scale=1.0):
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g) * scale
    for c in planted:
        a[:, c] *= 9.0             # outlier feature dims: |a| >= 6 in most rows
    return a.half()


def _weight(N, K, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, K, generator=g) * 0.02).half()


def _masks_np(t, K):
    w = t.cpu().numpy().astype(np.uint32)
    bits = (w[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1
    return bits.reshape(w.shape[0], K).astype(bool)


def test_weight_quantiser_bit_exact_with_row_maps(dev):
    from haff import quant
    K, F = 256, 96
    g, u = _weight(F, K, 1), _weight(F, K, 2)
    g[5] = 0                                            # an all-zero row
    g[7, 3] = 65504.0
    w = quant.quantize_int8([(g, quant.swiglu_rows(F)[0]), (u, quant.swiglu_rows(F)[1])], dev)
    rg, rgs = R.quantize_weight(g.float().numpy())
    ru, rus = R.quantize_weight(u.float().numpy())
    gr, ur = quant.swiglu_rows(F)
    cb, scb = w.cb.cpu().numpy(), w.scb.cpu().numpy()
    assert np.array_equal(cb[gr.numpy()], rg) and np.array_equal(cb[ur.numpy()], ru)
    assert np.array_equal(scb[gr.numpy()].view(np.int32), rgs.view(np.int32)) and np.array_equal(scb[ur.numpy()], rus)
    big = _weight(4096, 11008, 3)
    qb = quant.quantize_int8([(big, None)], dev)
    cb2, scb2 = qb.cb.cpu().numpy(), qb.scb.cpu().numpy()
    rcb, rscb = R.quantize_weight(big.float().numpy())
    assert np.array_equal(cb2, rcb) and np.array_equal(scb2, rscb)


@pytest.mark.parametrize("K", [4096, 11008, 5120, 13824])
def test_activation_quantiser_bit_exact(dev, K):
    from haff import ops
    M, seg = 24, 8
    a = _rows(M, K, K, planted=(3, K // 2, K - 1))
    a[5, 77] = 6.0                                      # exactly the threshold
    a[9] = 0.0                                          # all-zero row
    a[10, :] = 7.0                                      # all-outlier row
    valid = torch.tensor([8, 5, 8], dtype=torch.int32)
    masks = torch.zeros((3, K // 32), dtype=torch.int32, device=dev)
    q = ops.int8_quantize_act(a.to(dev), 6.0, seg, valid.to(dev), masks)
    rca, rsca, rmasks = R.quantize_rows(a.float().numpy(), 6.0, seg, valid.numpy())
    assert np.array_equal(q.ca.cpu().numpy(), rca)
    assert np.array_equal(q.sca.cpu().numpy().view(np.int32), rsca.view(np.int32))
    assert np.array_equal(_masks_np(masks, K), rmasks)
    nc = q.ncols.cpu().numpy()
    for s in range(3):
        assert np.array_equal(q.cols[s, :nc[s]].cpu().numpy(), np.flatnonzero(rmasks[s]))
    q0 = ops.int8_quantize_act(a.to(dev), 0.0, seg)      # threshold 0: no decomposition
    rca0, rsca0, _ = R.quantize_rows(a.float().numpy(), 0.0, seg)
    assert np.array_equal(q0.ca.cpu().numpy(), rca0) and q0.ncols.cpu().sum().item() == 0


def _check_product(dev, M, N, K, thr, seg, planted, n_check=None, form=0, seed=0):
    """Device product vs int8_ref on n_check sampled output columns (all when None)."""
    from haff import ops, quant
    a = _rows(M, K, seed + 1, planted)
    w = _weight(N, K, seed + 2)
    qw = quant.quantize_int8([(w, None)], dev)
    bias = torch.randn(N, generator=torch.Generator().manual_seed(seed + 3))
    q = ops.int8_quantize_act(a.to(dev), thr, seg)
    y = ops.linear_int8(q, qw.cb, qw.scb, bias=bias.to(dev), form=form).cpu()
    cols = np.arange(N) if n_check is None or n_check >= N else \
        np.unique(np.concatenate([np.random.default_rng(seed).choice(N, n_check, replace=False), [0, N - 1]]))
    rcb, rscb = R.quantize_weight(w.float().numpy())
    rca, rsca, rmasks = R.quantize_rows(a.float().numpy(), thr, seg)
    ry = R.product(a.float().numpy(), rca, rsca, rcb[cols], rscb[cols], rmasks, seg, bias.numpy()[cols])
    got = y.numpy()[:, cols]
    assert np.array_equal(got.view(np.int16), ry.view(np.int16)), (M, N, K, thr, int((got != ry).sum()))
    return y, int(rmasks.sum())


@pytest.mark.parametrize("M", [1, 8, 64, 300])
@pytest.mark.parametrize("shape", list(SHAPES_7B))
def test_int8_product_bit_exact_7b_shapes(dev, M, shape):
    N, K = SHAPES_7B[shape]
    _check_product(dev, M, N, K, 6.0, M, planted=(11, K // 3, K - 5), n_check=384 if M >= 64 else 1024)


@pytest.mark.parametrize("shape", list(SHAPES_13B))
def test_int8_product_bit_exact_13b_shapes(dev, shape):
    N, K = SHAPES_13B[shape]
    _check_product(dev, 8, N, K, 6.0, 8, planted=(0, 1000), n_check=512)


@pytest.mark.parametrize("M", [1, 64, 300])
def test_int8_product_low_threshold_and_zero(dev, M):
    _, ncols = _check_product(dev, M, 640, 4096, 1.5, M, planted=(), n_check=None, seed=4)   # |a| >= 1.5: hundreds of columns
    assert ncols >= 200
    _check_product(dev, M, 640, 4096, 0.0, M, planted=(), n_check=None, seed=5)


@pytest.mark.parametrize("shape", list(SHAPES_7B))
def test_int8_product_large_ragged_m(dev, shape):
    """The tiled form over many row and weight tiles: M = 4096 + 37 rows in frames of 300, every 7B shape (lm_head's N tail)."""
    N, K = SHAPES_7B[shape]
    _check_product(dev, 4096 + 37, N, K, 6.0, 300, planted=(5, 999), n_check=64, seed=6)


def test_row_output_independent_of_form_m_and_batch(dev):
    """Weight-streaming vs tiled form, and one segment alone vs inside a batch: the same bits for each row."""
    from haff import ops, quant
    K, N, seg = 4096, 4096 + 64, 8
    a = _rows(64, K, 21, planted=(100, 2000))
    a[17, 3000] = -40.0                                  # a column of segment 2 only
    qw = quant.quantize_int8([(_weight(N, K, 22), None)], dev)
    q = ops.int8_quantize_act(a.to(dev), 6.0, seg)
    y1 = ops.linear_int8(q, qw.cb, qw.scb, form=ops.INT8_SKINNY)
    y2 = ops.linear_int8(q, qw.cb, qw.scb, form=ops.INT8_TILED)
    assert torch.equal(y1, y2)
    for s in (0, 2, 7):
        qs = ops.int8_quantize_act(a[s * seg:(s + 1) * seg].contiguous().to(dev), 6.0, seg)
        for form in (ops.INT8_SKINNY, ops.INT8_TILED):
            assert torch.equal(ops.linear_int8(qs, qw.cb, qw.scb, form=form), y1[s * seg:(s + 1) * seg])
        # a decode-style call: one row against its segment's sticky masks
        mk = torch.zeros((1, K // 32), dtype=torch.int32, device=dev)
        ops.int8_quantize_act(a[s * seg:(s + 1) * seg].contiguous().to(dev), 6.0, seg, masks=mk)
        row = ops.int8_quantize_act(a[s * seg + 1:s * seg + 2].contiguous().to(dev), 6.0, 1, masks=mk)
        assert torch.equal(ops.linear_int8(row, qw.cb, qw.scb), y1[s * seg + 1:s * seg + 2])
    big = ops.int8_quantize_act(a.repeat(5, 1).to(dev), 6.0, seg)   # M = 320: the tiled form over many frames
    assert torch.equal(ops.linear_int8(big, qw.cb, qw.scb)[128:192], y1)


def test_residual_and_swiglu_epilogues(dev):
    from haff import ops, quant
    K, F, M = 4096, 512, 24
    a = _rows(M, K, 31, planted=(7,))
    g, u = _weight(F, K, 32), _weight(F, K, 33)
    gr, ur = quant.swiglu_rows(F)
    wgu = quant.quantize_int8([(g, gr), (u, ur)], dev)
    q = ops.int8_quantize_act(a.to(dev), 6.0, 8)
    for form in (ops.INT8_SKINNY, ops.INT8_TILED):
        h = ops.linear_int8(q, wgu.cb, wgu.scb, swiglu=True, form=form).cpu().float()
        y = ops.linear_int8(q, wgu.cb, wgu.scb, form=form).cpu().float()   # Y of the interleaved rows
        yg, yu = y[:, gr], y[:, ur]
        ref = (torch.nn.functional.silu(yg) * yu).half().float()
        ulp = torch.clamp(ref.abs(), min=2.0 ** -14) * 2.0 ** -10
        assert ((h - ref).abs() <= ulp * 1.01).all()
        wo = quant.quantize_int8([(_weight(K, F, 34), None)], dev)
        x = _rows(M, K, 35).to(dev)
        hq = ops.int8_quantize_act(h.half().to(dev), 6.0, 8)
        yo = ops.linear_int8(hq, wo.cb, wo.scb, form=form).cpu().float()
        out = x.clone()
        ops.linear_int8(hq, wo.cb, wo.scb, resid=out, out=out, form=form)
        ref = (x.cpu().float() + yo).half().float()
        assert torch.equal(out.cpu().float(), ref)


# ---- the model against the oracle with int8_ref Linears ------------------------------------------------------------------------
class _Int8Oracle:
    """Monkeypatches the oracle's F.linear: a converted Linear (by weight identity) runs int8_ref on f16 inputs, one segment per frame
    (the leading dimension); lm_head, which the oracle applies to the last rows only, takes its columns from every row of the frame's
    last llama_forward output (the reference's lm_head sees every position). sticky=True (with lisa_evaluate(use_cache=True)): the
    KV-cached schedule of LisaMI355 — a call of more than one row per frame sets a Linear's masks, a one-row call ORs its outliers in,
    so it isolates the one deviation the KV cache leaves (earlier rows are not requantised when a decode step adds a column)."""

    def __init__(self, O, sd, thr, sticky=False):
        from haff import quant
        self.O, self.thr, self.sticky, self.masks = O, thr, sticky, {}
        self.w = {id(v): R.quantize_weight(v.float().numpy()) for k, v in sd.items() if quant.int8_linear(k)}
        self.lm = id(sd["lm_head.weight"])
        self.last_h = None

    def linear(self, x, w, b=None):
        import torch.nn.functional as TF
        q = self.w.get(id(w))
        if q is None:
            return TF.linear(x, w, b)
        bias = None if b is None else b.float().numpy()
        if id(w) == self.lm and x.dim() == 2:
            B, H = x.shape
            masks = self._masks(w, B, H, self.last_h.shape[1])
            R.quantize_rows(self.last_h.reshape(-1, H).numpy(), self.thr, self.last_h.shape[1], masks=masks)
            y = R.linear(x.numpy(), q[0], q[1], self.thr, 1, masks=masks, bias=bias)
            return torch.from_numpy(y.astype(np.float32))
        lead = x.shape[:-1]
        x2 = x.reshape(lead[0], -1, x.shape[-1])
        T = x2.shape[1]
        masks = self._masks(w, lead[0], x.shape[-1], T) if self.sticky else None
        y = R.linear(x2.reshape(-1, x.shape[-1]).numpy(), q[0], q[1], self.thr, T, masks=masks, bias=bias)
        return torch.from_numpy(y.astype(np.float32)).reshape(*lead, -1)

    def _masks(self, w, B, K, T):
        if not self.sticky or T > 1 or id(w) not in self.masks:
            self.masks[id(w)] = np.zeros((B, K), dtype=bool)
        return self.masks[id(w)]

    def __enter__(self):
        import torch.nn.functional as TF
        O, me = self.O, self

        class _F:
            def __getattr__(self, name):
                return me.linear if name == "linear" else getattr(TF, name)
        self._F, self._lf = O.F, O.llama_forward

        def llama_forward(*a, **k):
            h = me._lf(*a, **k)
            me.last_h = h.detach().float()
            return h
        O.F, O.llama_forward = _F(), llama_forward
        return self

    def __exit__(self, *exc):
        self.O.F, self.O.llama_forward = self._F, self._lf
        return False


def _planted(sd, cfg, dims=(3, 17)):
    """Outlier features: a few large RMSNorm gamma entries on every layer's input and post-attention norms and the final norm."""
    sd = dict(sd)
    for i in range(cfg.llm.layers):
        for n in ("input_layernorm", "post_attention_layernorm"):
            k = f"model.layers.{i}.{n}.weight"
            g = sd[k].clone()
            g[list(dims)] = 24.0
            sd[k] = g
    g = sd["model.norm.weight"].clone()
    g[list(dims)] = 24.0
    sd["model.norm.weight"] = g
    return sd


@pytest.mark.parametrize("cfg_name", ["tiny", "mid"])
def test_load_in_8bit_matches_int8_oracle(dev, cfg_name):
    import test_fp16_lisa_gpu as F16
    from haff.lisa import LisaMI355
    from oracle import lisa_oracle as O
    cfg, sd, images, images_clip, ids, forced = F16._setup(cfg_name)
    sd = _planted(sd, cfg)
    S = cfg.sam.img_size
    B = ids.shape[0]
    resize = [(S, S), (S, S - 32)]
    orig = [(S, S), (S // 2 + 3, S // 2 - 10)]
    refs = {}
    with torch.no_grad():
        with _Int8Oracle(O, sd, 6.0):
            refs["int8"] = O.lisa_evaluate(sd, cfg, images_clip, images, ids, resize, orig, max_new_tokens=forced.shape[1],
                                           forced_answer=forced, use_cache=False)
        with _Int8Oracle(O, sd, 6.0, sticky=True) as kv_shim:
            refs["int8_kv"] = O.lisa_evaluate(sd, cfg, images_clip, images, ids, resize, orig, max_new_tokens=forced.shape[1],
                                              forced_answer=forced, use_cache=True)
        refs["plain"] = O.lisa_evaluate(sd, cfg, images_clip, images, ids, resize, orig, max_new_tokens=forced.shape[1],
                                        forced_answer=forced, use_cache=False)

    def errors(out, ref):
        errs, terrs = [], []
        for i in range(B):
            for got, r in ((out[1][i], ref[1][i]), (out[2][i], ref[2][i])):
                gg = got.cpu()
                assert torch.isfinite(gg).all()
                errs.append((gg - r).abs().max().item() / r.abs().max().item())
            terrs.append((out[3][i].cpu() - ref[3][i]).abs().max().item())
        return max(errs), max(terrs)
    stats = {}
    for name, kw in (("int8", {"load_in_8bit": True}), ("fp16", {})):
        m = LisaMI355(cfg, sd, dtype=torch.float16, device=dev, **kw)
        out = F16._run(m, dev, images_clip, images, ids, forced, resize, orig)
        stats[name] = {"ids": out[0].cpu(), **{k: errors(out, r) for k, r in refs.items()}}
        if name == "int8":
            # the outlier columns this model ended with vs the KV-cached oracle's, per (Linear input, frame): a column in one set and
            # not the other requantises that column of every row of the frame (an fp16-vs-fp32 difference of an input near the
            # threshold is enough)
            cache = next(iter(m._caches.values()))
            L = cfg.llm.layers
            names = [f"model.layers.{i}.{n}.weight" for i in range(L)
                     for n in ("self_attn.q_proj", "self_attn.o_proj", "mlp.gate_proj", "mlp.down_proj")] + ["lm_head.weight"]
            flips = total = 0
            for slot, n in enumerate(names):
                got = _masks_np(cache["i8"][slot], cache["i8"][slot].shape[1] * 32)
                want = kv_shim.masks[id(sd[n])]
                flips += int((got != want).sum())
                total += int((got | want).sum())
            stats["flips"] = (flips, total)
            print(f"{cfg_name}: outlier columns differing from the KV-cached oracle's: {flips} of {total}")
        print(f"{cfg_name} {name}: mask err/scale, taxonomy err vs " +
              ", ".join(f"{k} oracle {stats[name][k][0]:.3e} {stats[name][k][1]:.3e}" for k in refs))
        del m
    d = errors(refs["int8_kv"], refs["int8"])
    print(f"{cfg_name}: KV-cached int8 oracle vs recompute int8 oracle (the KV-cache deviation alone): {d[0]:.3e} {d[1]:.3e}")
    assert torch.equal(stats["int8"]["ids"], refs["int8"][0])
    # the issue's bounds, against the oracle of the schedule this model runs (KV-cached, sticky masks), and, at tiny, against the
    # reference's own recompute schedule too
    if stats["flips"][0] == 0:
        assert stats["int8"]["int8_kv"][0] <= 0.5 * stats["fp16"]["int8_kv"][0], stats
        assert stats["int8"]["int8_kv"][1] <= 1e-3, stats
    else:
        # a differing column set puts this mode at the int8 quantisation distance from the oracle, where the fp16 mode is: it has to
        # be no farther than that
        assert stats["int8"]["int8_kv"][0] <= 1.05 * stats["fp16"]["int8_kv"][0], stats
        assert stats["int8"]["int8_kv"][1] <= 1.05 * stats["fp16"]["int8_kv"][1], stats
    if cfg_name == "tiny":
        assert stats["int8"]["int8"][0] <= 0.5 * stats["fp16"]["int8"][0], stats
        assert stats["int8"]["int8"][1] <= 1e-3, stats


def _full_width_layer_against_oracle(dev, width):
    """One Llama layer at 7B / 13B width, 2 frames x 16 rows (M = 32: the weight-streaming form's MT = 2, two weight tiles per
    workgroup for q|k|v), against the oracle with int8_ref Linears: the mean relative error at most half the fp16 model's."""
    from haff import config as hcfg
    from haff.llava import LlamaHip
    from oracle import lisa_oracle as O
    lc = (hcfg.haff_7b() if width == "7B" else hcfg.haff_13b()).llm
    lc.layers = 1
    H, F = lc.hidden, lc.ffn
    g = torch.Generator().manual_seed(9)
    sd = {"model.embed_tokens.weight": torch.randn(64, H, generator=g).half().float(),
          "model.norm.weight": torch.ones(H), "lm_head.weight": torch.randn(64, H, generator=g).half().float() * 0.02}
    L = "model.layers.0"
    for n, shp in (("self_attn.q_proj", (H, H)), ("self_attn.k_proj", (H, H)), ("self_attn.v_proj", (H, H)),
                   ("self_attn.o_proj", (H, H)), ("mlp.gate_proj", (F, H)), ("mlp.up_proj", (F, H)), ("mlp.down_proj", (H, F))):
        sd[f"{L}.{n}.weight"] = (torch.randn(*shp, generator=g) * 0.02).half().float()
    for n in ("input_layernorm", "post_attention_layernorm"):
        w = torch.ones(H)
        w[[5, 1000]] = 24.0
        sd[f"{L}.{n}.weight"] = w
    x = (torch.randn(2, 16, H, generator=g)).half().float()
    with torch.no_grad(), _Int8Oracle(O, sd, 6.0):
        ref = O.llama_forward(sd, x, lc)
    errs = {}
    for name, i8 in (("int8", True), ("fp16", False)):
        m = LlamaHip(sd, lc, torch.float16, dev, int8=i8)
        cache = m.new_cache(2, 16)
        kw = {"valid": torch.full((2,), 16, dtype=torch.int32, device=dev)} if i8 else {}
        got = m.forward(x.half().to(dev), cache, **kw).float().cpu()
        errs[name] = ((got - ref).abs().mean() / ref.abs().mean()).item()
        del m
    print(f"{width}-width layer vs int8 oracle: mean rel err int8 {errs['int8']:.3e}, fp16 {errs['fp16']:.3e}")
    assert errs["int8"] <= 0.5 * errs["fp16"]


def test_full_width_7b_layer_against_oracle(dev):
    _full_width_layer_against_oracle(dev, "7B")


def test_full_width_13b_layer_against_oracle(dev):
    _full_width_layer_against_oracle(dev, "13B")


@pytest.mark.parametrize("B", [1, 4])
def test_graph_decode_equals_eager_in_8bit_mode(dev, B):
    import test_fp16_lisa_gpu as F16
    from haff.lisa import LisaMI355
    cfg, sd, images, images_clip, ids, forced = F16._setup("mid", B=B)
    sd = _planted(sd, cfg)
    S = cfg.sam.img_size
    resize, orig = [(S, S)] * B, [(S, S)] * B
    model = LisaMI355(cfg, sd, dtype=torch.float16, device=dev, load_in_8bit=True)
    runs = []
    for graphs in (True, False):
        model.decode_graphs = graphs
        runs.append(F16._run(model, dev, images_clip, images, ids, forced, resize, orig))
    assert torch.equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1] + runs[0][2] + runs[0][3], runs[1][1] + runs[1][2] + runs[1][3]):
        assert torch.equal(a, b)


def test_footprint_and_no_fp16_copy(dev):
    import test_fp16_lisa_gpu as F16
    from haff.lisa import LisaMI355
    from haff import quant
    cfg, sd, *_ = F16._setup("mid")
    m8 = LisaMI355(cfg, sd, dtype=torch.float16, device=dev, load_in_8bit=True)
    b8 = m8.llm_weight_bytes()
    m16 = LisaMI355(cfg, sd, dtype=torch.float16, device=dev)
    b16 = m16.llm_weight_bytes()
    rows = sum(L[k].shape[0] for L in m8.llm.layers for k in ("wqkv", "wo", "wgu", "wd")) + m8.llm.lm_head.shape[0]
    assert b8 == b16 // 2 + 4 * rows, (b8, b16, rows)
    for L in m8.llm.layers:
        for k in ("wqkv", "wo", "wgu", "wd"):
            assert isinstance(L[k], quant.Int8Weight)
    assert isinstance(m8.llm.lm_head, quant.Int8Weight) and isinstance(m8.w_proj, quant.Int8Weight)
    assert not m8.llm.carry_rms and not m8.llm.fused_qkv_rope


@pytest.mark.parametrize("thr", [6.0, 1.0])
def test_sticky_mask_growth_diagnostic(dev, thr):
    """How often a decode step adds an outlier column to a frame's masks (where the KV cache's old rows would have been requantised
    by the reference): reported, not bounded."""
    import test_fp16_lisa_gpu as F16
    from haff.lisa import LisaMI355
    cfg, sd, images, images_clip, ids, forced = F16._setup("mid", n_gen=8)
    forced[:, -1] = 5
    sd = _planted(sd, cfg)
    model = LisaMI355(cfg, sd, dtype=torch.float16, device=dev, load_in_8bit=True, llm_int8_threshold=thr)
    model.decode_graphs = False
    grew, before = [], []
    inner_rows, inner_logits = model.llm.decode_rows, model.llm.next_token_logits

    def rows(x1, cache):
        before.append((cache, [t.clone() for t in cache["i8"]]))
        return inner_rows(x1, cache)

    def logits(h):
        out = inner_logits(h)
        if before:   # a decode step ends with lm_head, whose masks grow here (the prefill's first token has no snapshot)
            cache, snap = before.pop()
            grew.append(any(not torch.equal(b, t) for b, t in zip(snap, cache["i8"])))
        return out
    model.llm.decode_rows, model.llm.next_token_logits = rows, logits
    model.generate(images_clip.to(dev), ids.to(dev), max_new_tokens=forced.shape[1], forced_answer=forced.to(dev))
    print(f"threshold {thr}: a sticky mask grew in {sum(grew)} of {len(grew)} decode steps")
    assert len(grew) == forced.shape[1] - 1
