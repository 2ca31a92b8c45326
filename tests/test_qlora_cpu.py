"""NF4 fine-tuning (QLoRA), host side (no GPU): train_ds.py's --load_in_4bit / --load_in_8bit flags and their exits, LisaTrainable's
option refusals, and the declaration and ctypes prototype of haff_nf4_dequant_t_f16 (its host-side refusals:
tests/test_quant_contract_cpu.py)."""
import ctypes
import os
import re

import pytest
import torch

import haff

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_train_ds_parses_the_quantisation_flags():
    from haff import train_ds
    a = train_ds.parse_args([])
    assert a.load_in_4bit is False and a.load_in_8bit is False
    a = train_ds.parse_args(["--load_in_4bit", "--precision", "fp16"])
    assert a.load_in_4bit is True and a.load_in_8bit is False
    assert train_ds.parse_args(["--load_in_8bit"]).load_in_8bit is True


@pytest.mark.parametrize("precision", ["bf16", "fp32", None])
def test_train_ds_4bit_needs_fp16(precision):
    """exits before any device is touched (this machine has none: a later check would raise the 'needs MI355X' exit instead)"""
    from haff import train_ds
    argv = ["--synthetic", "tiny", "--load_in_4bit"] + (["--precision", precision] if precision else [])
    with pytest.raises(SystemExit) as e:
        train_ds.main(argv)
    assert "--load_in_4bit requires --precision fp16" in str(e.value)


@pytest.mark.parametrize("extra", [[], ["--precision", "fp16"], ["--precision", "fp16", "--load_in_4bit"]])
def test_train_ds_8bit_is_not_built_for_training(extra):
    from haff import train_ds
    with pytest.raises(SystemExit) as e:
        train_ds.main(["--synthetic", "tiny", "--load_in_8bit"] + extra)
    assert "not built for training" in str(e.value) and "\n" not in str(e.value)


def test_trainer_load_in_4bit_option_refusals():
    """as tests/test_nf4_cpu.py::test_load_in_4bit_option_refusals for the inference class: ValueError before any device work"""
    from haff import config as hcfg
    from haff.train_model import LisaTrainable
    cfg = hcfg.tiny()
    with pytest.raises(ValueError, match="float16"):
        LisaTrainable(cfg, {}, dtype=torch.bfloat16, load_in_4bit=True)
    with pytest.raises(ValueError, match="float16"):
        LisaTrainable(cfg, {}, dtype=torch.float32, load_in_4bit=True)
    with pytest.raises(ValueError, match="float16"):
        LisaTrainable(cfg, {}, load_in_4bit=True)   # the default dtype is bf16
    with pytest.raises(ValueError, match="fp4"):
        LisaTrainable(cfg, {}, dtype=torch.float16, load_in_4bit=True, bnb_4bit_quant_type="fp4")


def _c_args(decl):
    """ctypes types of a C parameter list as include/haff_hip.h writes them"""
    out = []
    for a in decl.split(","):
        a = " ".join(a.split())
        if "*" in a:
            out.append(ctypes.c_void_p)
        elif a.startswith("long "):
            out.append(ctypes.c_long)
        elif a.startswith("int "):
            out.append(ctypes.c_int)
        elif a.startswith("float "):
            out.append(ctypes.c_float)
        else:
            raise AssertionError(a)
    return out


def test_dequant_t_declared_with_the_same_signature_in_header_and_ctypes_table():
    from haff import lib
    text = open(os.path.join(ROOT, "include", "haff_hip.h")).read()
    m = re.search(r"^int haff_nf4_dequant_t_f16\(([^)]*)\);", text, flags=re.M)
    assert m, "haff_nf4_dequant_t_f16 is not declared in include/haff_hip.h"
    assert "haff_nf4_dequant_t_f16" in haff.EXPORTED_SYMBOLS
    assert _c_args(m.group(1)) == lib._PROTOS["haff_nf4_dequant_t_f16"]
    # ... and it is haff_nf4_dequant_f16's signature: the same arguments, the output transposed
    m0 = re.search(r"^int haff_nf4_dequant_f16\(([^)]*)\);", text, flags=re.M)
    assert _c_args(m0.group(1)) == _c_args(m.group(1)) == lib._PROTOS["haff_nf4_dequant_f16"]


def test_nf4_weight_has_dequant_t():
    from haff import quant
    assert callable(getattr(quant.Nf4Weight, "dequant_t", None))
