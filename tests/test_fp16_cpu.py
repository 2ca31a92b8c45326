"""fp16 inference mode, host side (no GPU): the --precision mapping of the CLIs, the flags that still exit, the *_f16 entry points
of the C-ABI (declared, exported, and refusing shapes they do not take before anything is launched)."""
import ctypes
import os
import re

import pytest
import torch

import haff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16_SYMBOLS = ("haff_gemm_f16", "haff_gemm_f16_cfg", "haff_gemm_f16_ws", "haff_attention_f16", "haff_attention_decode_rows_f16",
               "haff_decode_attention_rope_rows_f16")


def test_precision_maps_to_the_model_dtype():
    from haff import inference
    assert inference.precision_dtype("fp16") == torch.float16
    assert inference.precision_dtype("bf16") == torch.bfloat16
    assert inference.precision_dtype("fp32") == torch.float32
    assert inference.parse_args(["--precision", "fp16"]).precision == "fp16"
    with pytest.raises(SystemExit):
        inference.precision_dtype("fp8")


@pytest.mark.parametrize("flag", ["--load_in_8bit", "--load_in_4bit"])
def test_quantised_loading_still_exits(flag):
    from haff import inference
    args = inference.parse_args([flag, "--precision", "fp16", "--synthetic", "tiny"])
    with pytest.raises(SystemExit, match="bitsandbytes"):
        inference.build_model_and_tokenizer(args)


def test_f16_entry_points_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "haff_hip.h")).read()
    declared = set(re.findall(r"^int (haff_\w+)\(", text, flags=re.M))
    if not os.path.exists(haff.LIB_PATH):
        haff.build_library()
    lib = ctypes.CDLL(haff.LIB_PATH)
    for name in F16_SYMBOLS:
        assert name in declared and name in haff.EXPORTED_SYMBOLS, name
        assert hasattr(lib, name), name


def test_f16_entry_points_refuse_bad_shapes_on_the_host():
    """Every refusal below happens in the host dispatcher before a kernel is enqueued (null device pointers are never touched):
    -1 bad argument, -2 a geometry the kernels do not serve."""
    lib = haff.load_library()
    fake = 0x1000   # 16-B aligned, never dereferenced
    gemm = [fake, 16, fake, 16, fake, 16, None, None, 0, None]
    assert int(lib.haff_gemm_f16(*gemm, 0, 16, 16, 0, 0, 0, None)) == -1            # M = 0
    assert int(lib.haff_gemm_f16(*gemm, 16, 16, 12, 0, 0, 0, None)) == -1           # K % 8
    assert int(lib.haff_gemm_f16_cfg(*gemm, 16, 48, 16, 0, 0, 1, 0, None)) == -1    # SwiGLU needs N % 32 == 0
    assert int(lib.haff_gemm_f16_ws(*gemm, 64, 16, 16, 0, 0, 0, fake + 8, 1 << 20, None)) == -1   # misaligned workspace
    st = [fake, 0, 0, 64]

    def attn(B, H, Nq, Nk, d, causal, relh, relw, S):
        return int(lib.haff_attention_f16(*st, *st, *st, *st, B, H, Nq, Nk, d, 0.125, causal, 0, relh, relw, S, None))
    assert attn(1, 1, 16, 16, 136, 0, None, None, 0) == -1          # d > 128
    assert attn(1, 1, 1600, 1600, 64, 1, fake, fake, 40) == -1      # rel-pos bias with a causal mask
    assert attn(1, 1, 1600, 1600, 64, 0, fake, fake, 40) == -2      # rel-pos grid of 40: neither S == 64 nor S <= 32
    assert int(lib.haff_attention_decode_rows_f16(fake, 0, 128, fake, 0, 128, 128, fake, 0, 128, 128, fake, 0, 128,
                                                  1, 1, 8, 128, 0.1, None, None)) == -1   # nk_rows required
    assert int(lib.haff_decode_attention_rope_rows_f16(fake, 384, fake, fake, fake, fake, 1, 1, 64, 16, 0.1, fake, None)) == -1  # d != 128
