"""The LLM.int8 8-bit mode's host side (no GPU): hand cases of the independent restatement (tests/int8_ref.py), haff.quant's
restatement against it, the option refusals, and the three entry points' declarations (their host-side refusals:
tests/test_quant_contract_cpu.py)."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

import haff
from haff import quant as Q

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))   # tests/int8_ref.py
import int8_ref as R   # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("haff_int8_quantize_weight_f16", "haff_int8_quantize_act_f16", "haff_gemm_int8_f16")


class _Quant:
    """haff.quant's CPU restatement behind int8_ref's numpy interface: the hand fixtures below pin both."""
    C = R.C

    @staticmethod
    def quantize_weight(w):
        cb, scb = Q.int8_quantize_weight_cpu(torch.as_tensor(np.asarray(w, dtype=np.float32)))
        return cb.numpy(), scb.numpy()

    @staticmethod
    def quantize_rows(a, threshold, seg_rows=None, valid=None, masks=None):
        tm = None if masks is None else torch.from_numpy(masks)      # shares memory: ORed in place like int8_ref's
        ca, sca, cols = Q.int8_quantize_rows_cpu(torch.as_tensor(np.asarray(a, dtype=np.float32)), threshold, seg_rows,
                                                 None if valid is None else torch.as_tensor(valid), tm)
        return ca.numpy(), sca.numpy(), cols.numpy()

    @staticmethod
    def product(a, ca, sca, cb, scb, masks, seg_rows=None, bias=None):
        t = torch.from_numpy
        return Q.int8_linear_cpu(t(np.asarray(a, dtype=np.float32)), t(cb), t(scb), t(ca), t(sca), t(masks), seg_rows,
                                 None if bias is None else t(np.asarray(bias, dtype=np.float32))).numpy()


@pytest.fixture(params=["int8_ref", "quant"])
def R(request):   # noqa: F811  (each hand fixture runs on both restatements)
    return sys.modules["int8_ref"] if request.param == "int8_ref" else _Quant


def test_worked_example(R):
    """[1, -2, 7, 0.5] at threshold 6: column 2 is an outlier, SCA = 2, scale 63.5, codes [64, -127, 0, 32] (63.5 -> 64 and
    31.75 -> 32)."""
    ca, sca, masks = R.quantize_rows(np.array([[1, -2, 7, 0.5]]), 6.0)
    assert ca.tolist() == [[64, -127, 0, 32]] and sca.tolist() == [2.0] and masks.tolist() == [[False, False, True, False]]


def test_rint_ties_go_to_even(R):
    # SCA 127: scale 1, so the codes are rint of the values themselves
    ca, _, _ = R.quantize_rows(np.array([[127, 0.5, 1.5, 2.5, -0.5, -1.5, -2.5, 3.5]]), 0.0)
    assert ca.tolist() == [[127, 0, 2, 2, 0, -2, -2, 4]]
    cb, scb = R.quantize_weight(np.array([[-127, 0.5, 1.5, -2.5]]))
    assert cb.tolist() == [[-127, 0, 2, -2]] and scb.tolist() == [127.0]


def test_threshold_edges(R):
    a = np.array([[6.0, 1.0, -5.99609375, 2.0], [0.5, -6.0, 1.0, 0.25]])
    ca, sca, masks = R.quantize_rows(a, 6.0)
    assert masks.tolist() == [[True, True, False, False]]                 # |a| = 6.0 counts; column 1 from row 1
    assert sca.tolist() == [5.99609375, 1.0]
    assert ca[:, :2].tolist() == [[0, 0], [0, 0]]                         # outlier columns are zero in EVERY row of the segment
    ca0, sca0, masks0 = R.quantize_rows(a, 0.0)                           # threshold 0: no decomposition
    assert not masks0.any() and sca0.tolist() == [6.0, 6.0] and ca0[0, 0] == 127 and ca0[1, 1] == -127


def test_all_outlier_and_all_zero_rows(R):
    ca, sca, masks = R.quantize_rows(np.array([[7, -8, 9, 10], [0, 0, 0, 0], [1, 0, 0, 0]]), 6.0)
    assert sca.tolist() == [0.0, 0.0, 1.0] and not ca[:2].any() and ca[2].tolist() == [0, 0, 0, 0]   # column 0 is an outlier column
    cb, scb = R.quantize_weight(np.zeros((1, 64)))
    assert scb.tolist() == [0.0] and not cb.any()


def test_segments_and_padding_rows(R):
    a = np.ones((6, 4))
    a[0, 1] = 9         # frame 0, valid row
    a[2, 3] = 9         # frame 0, padding row (valid 2 of 3): not a column of frame 0
    a[4, 2] = -7        # frame 1
    ca, sca, masks = R.quantize_rows(a, 6.0, seg_rows=3, valid=[2, 3])
    assert masks.tolist() == [[False, True, False, False], [False, False, True, False]]
    assert ca[1].tolist() == [127, 0, 127, 127] and ca[3].tolist() == [127, 127, 0, 127]
    assert ca[2].tolist() == [127, 0, 127, 0]    # the padding row: its own outlier and its frame's columns are zero


def test_sticky_masks_accumulate(R):
    masks = np.zeros((1, 4), dtype=bool)
    R.quantize_rows(np.array([[1, 9, 1, 1]]), 6.0, masks=masks)
    ca, _, masks = R.quantize_rows(np.array([[1, 1, 1, -9], [2, 2, 2, 2]]), 6.0, masks=masks)
    assert masks.tolist() == [[False, True, False, True]] and ca[1].tolist() == [127, 0, 127, 0]


def test_outlier_product_by_hand(R):
    """One row, K = 2: code product, dequantisation and the outlier column's f16 term."""
    a = np.array([[8.0, 1.0]])
    w = np.array([[0.5, -1.0], [2.0, 4.0]])
    cb, scb = R.quantize_weight(w)
    assert cb.tolist() == [[64, -127], [64, 127]]
    ca, sca, masks = R.quantize_rows(a, 6.0)
    assert ca.tolist() == [[0, 127]] and masks.tolist() == [[True, False]]
    y = R.product(a, ca, sca, cb, scb, masks)
    t = np.float32(127 * -127) * R.C * np.float32(1.0) * np.float32(1.0)
    sub = np.float16(np.float32(64) * np.float32(1.0) / np.float32(127))
    expect0 = np.float16(np.float32(np.float16(t)) + np.float32(np.float16(np.float32(8.0) * np.float32(sub))))
    assert y[0, 0] == expect0 and abs(float(y[0, 0]) - (8 * 0.5 - 1)) < 0.05   # (0.5 is stored as 64 / 127)



def test_epilogue_by_hand():
    """int8_ref.epilogue: act on the f16 Y in fp32, + resid in fp32, one rounding to f16 (or none for fp32 out), the row map."""
    R = sys.modules["int8_ref"]
    y = np.array([[1.5, -2.0, 65504.0], [0.0009765625, -0.5, 3.0]], dtype=np.float16)
    assert np.array_equal(R.epilogue(y), y)
    assert R.epilogue(y, R.ACT_RELU).tolist() == [[1.5, 0.0, 65504.0], [0.0009765625, 0.0, 3.0]]
    # 2049 + 1 = 2050 in fp32 then f16 (spacing 2 above 2048): exact; 2048 + 1 in fp32 is 2049 -> ties to even 2048 in f16
    r = np.array([[2049.0, 1.0, -65504.0], [2048.0, 0.5, 1.0]], dtype=np.float16)
    y2 = np.array([[1.0, 1.0, 0.0], [1.0, 0.5, 0.0]], dtype=np.float16)
    assert R.epilogue(y2, resid=r).tolist() == [[2048.0, 2.0, -65504.0], [2048.0, 1.0, 1.0]]
    # fp32 out keeps 2048 + 1 and the overflow of an f16 sum
    assert R.epilogue(y2, resid=r.astype(np.float32), out_f32=True).tolist() == [[2049.0, 2.0, -65504.0], [2049.0, 1.0, 1.0]]
    with np.errstate(over="ignore"):
        assert np.isinf(R.epilogue(np.array([[65504.0]], np.float16), resid=np.array([[32.0]], np.float16))[0, 0])
    # the row map sends row 0 to output row 2, drops row 1, and the residual is read at the output row
    out = np.full((3, 3), 7.0, dtype=np.float16)
    res = np.arange(9, dtype=np.float16).reshape(3, 3)
    got = R.epilogue(y, resid=res, row_map=[2, -1], out=out)
    assert got.tolist() == [[7.0] * 3, [7.0] * 3, [7.5, 5.0, 65504.0]]
    # the transcendental acts are the exact functions of their fp32 input, rounded once
    x = np.array([[-3.0, -1.0, 0.0, 0.5, 2.0]], dtype=np.float16)
    assert np.allclose(R.epilogue(x, R.ACT_SILU, out_f32=True), x / (1 + np.exp(-x.astype(np.float64))), rtol=1e-7)
    assert np.allclose(R.epilogue(x, R.ACT_GELU, out_f32=True)[0], [-0.0040496940948904, -0.15865525393145707, 0.0, 0.34573123063700656,
                                                                 1.9544997361036416], rtol=1e-7)
    assert np.allclose(R.epilogue(x, R.ACT_QUICK_GELU, out_f32=True), x / (1 + np.exp(-1.702 * x.astype(np.float64))), rtol=1e-7)
    # SwiGLU: output column 16 j + i = silu(Y[32 j + i]) * Y[32 j + 16 + i]
    y3 = np.zeros((1, 64), dtype=np.float16)
    y3[0, 3], y3[0, 19], y3[0, 32], y3[0, 48] = 2.0, 3.0, -1.0, 4.0
    s = R.epilogue(y3, swiglu=True, out_f32=True)
    assert s.shape == (1, 32) and np.count_nonzero(s) == 2
    assert np.isclose(s[0, 3], 2 / (1 + np.exp(-2.0)) * 3, rtol=1e-7) and np.isclose(s[0, 16], -1 / (1 + np.exp(1.0)) * 4, rtol=1e-7)

@pytest.mark.parametrize("thr", [6.0, 1.5, 0.0])
def test_quant_module_agrees_with_restatement(thr):
    R = sys.modules["int8_ref"]
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(40, 128, generator=g) * 0.05).half()
    a = torch.randn(10, 128, generator=g).half()
    a[:, 7] *= 12
    a[3, 100] = -20
    cb, scb = Q.int8_quantize_weight_cpu(w)
    rcb, rscb = R.quantize_weight(w.float().numpy())
    assert np.array_equal(cb.numpy(), rcb) and np.array_equal(scb.numpy(), rscb)
    valid = [4, 3]
    ca, sca, cols = Q.int8_quantize_rows_cpu(a, thr, seg_rows=5, valid=valid)
    rca, rsca, rmasks = R.quantize_rows(a.float().numpy(), thr, seg_rows=5, valid=valid)
    assert np.array_equal(ca.numpy(), rca) and np.array_equal(sca.numpy(), rsca) and np.array_equal(cols.numpy(), rmasks)
    bias = torch.randn(40, generator=g)
    y = Q.int8_linear_cpu(a, cb, scb, ca, sca, cols, seg_rows=5, bias=bias)
    ry = R.product(a.float().numpy(), rca, rsca, rcb, rscb, rmasks, seg_rows=5, bias=bias.numpy())
    assert np.array_equal(y.numpy().view(np.int16), ry.view(np.int16))


def test_module_selection_is_the_4bit_one():
    for name in ("model.layers.3.self_attn.q_proj.weight", "model.layers.0.mlp.down_proj.weight", "model.mm_projector.weight",
                 "model.text_hidden_fcs.0.2.weight", "lm_head.weight"):
        assert Q.int8_linear(name)
    for name in ("model.embed_tokens.weight", "model.norm.weight", "model.visual_model.image_encoder.blocks.0.attn.qkv.weight",
                 "model.layers.0.input_layernorm.weight", "model.mm_projector.bias"):
        assert not Q.int8_linear(name)
    assert not Q.int8_linear("lm_head.weight", lm_head=False)


def test_load_in_8bit_option_refusals():
    from haff import config as hcfg
    from haff.lisa import LisaMI355
    cfg = hcfg.tiny()
    with pytest.raises(ValueError, match="float16"):
        LisaMI355(cfg, {}, dtype=torch.bfloat16, load_in_8bit=True)
    with pytest.raises(ValueError, match="exclusive"):
        LisaMI355(cfg, {}, dtype=torch.float16, load_in_8bit=True, load_in_4bit=True)
    with pytest.raises(ValueError, match="has_fp16_weight"):
        LisaMI355(cfg, {}, dtype=torch.float16, load_in_8bit=True, llm_int8_has_fp16_weight=True)
    with pytest.raises(ValueError, match="threshold"):
        LisaMI355(cfg, {}, dtype=torch.float16, load_in_8bit=True, llm_int8_threshold=-1.0)


def test_int8_entry_points_declared():
    """(their host-side refusals: tests/test_quant_contract_cpu.py)"""
    text = open(os.path.join(ROOT, "include", "haff_hip.h")).read()
    for name in ENTRY:
        assert re.search(r"^int %s\(" % name, text, flags=re.M), name
        assert name in haff.EXPORTED_SYMBOLS
    if not os.path.exists(haff.LIB_PATH):
        haff.build_library()
    assert all(hasattr(ctypes.CDLL(haff.LIB_PATH), n) for n in ENTRY)
