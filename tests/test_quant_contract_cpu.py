"""The NF4 and int8 entry points' host-side contract (no GPU): which inputs each one refuses, and with WHICH code — -1 (bad argument)
or -2 (a geometry the kernels do not serve). The order of the checks is part of the contract: an input that breaks a -1 rule and a
-2 rule at once gets the code of the rule checked first. The two families order them differently: haff_gemm_nf4_*_f16 asks for
M > 64 (-2) right after the zero dimensions, AHEAD of every other -1 rule, haff_gemm_int8_f16 asks for form = 1 with M > 64 (-2) LAST.
Every case below is refused before anything is launched (the addresses are fake, 16-byte aligned and never dereferenced); no case
would pass validation. The expected codes were recorded from the library as it stood before the host halves of gemm_nf4.hip and
gemm_int8.hip were reorganised around csrc/gemm_quant.h; they are not derived from the code under test.

The cases that tests/test_nf4_cpu.py, test_qlora_cpu.py, test_lora_serve_cpu.py and test_int8_cpu.py used to probe are all here
(marked "was: <file>"); those files keep their tests of the declarations, the restatements and the options."""
import os

import pytest

import haff

F = 0x1000          # 16-byte aligned, never dereferenced
ODD = F + 8         # 8-byte aligned only
BAD, UNS = -1, -2
NAN = float("nan")

NF4_GEMM = ("A", "lda", "Wq", "absmax", "C", "ldc", "bias", "resid", "ldr", "row_map", "M", "N", "K", "act", "out_f32", "swiglu")
NF4_GEMM_BASE = dict(A=F, lda=64, Wq=F, absmax=F, C=F, ldc=64, bias=None, resid=None, ldr=64, row_map=None, M=1, N=64, K=64, act=0,
                     out_f32=0, swiglu=0, stream=None)
DEQ = ("packed", "absmax", "N", "K", "row_map", "out", "ldo")
DEQ_BASE = dict(packed=F, absmax=F, N=16, K=64, row_map=None, out=F, ldo=64, stream=None)

# entry point -> (argument order, a base argument set that every case below spoils)
ENTRY = {
    "haff_nf4_quantize_f16": (("W", "ldw", "N", "K", "double_quant", "row_map", "packed", "absmax", "offset", "workspace",
                               "workspace_bytes", "stream"),
                              dict(W=F, ldw=64, N=16, K=64, double_quant=1, row_map=None, packed=F, absmax=F, offset=F, workspace=F,
                                   workspace_bytes=1 << 20, stream=None)),
    "haff_nf4_dequant_f16": (DEQ + ("stream",), DEQ_BASE),
    "haff_nf4_dequant_t_f16": (DEQ + ("stream",), dict(DEQ_BASE, ldo=16)),       # K rows of roundup(N, 8) columns
    "haff_nf4_dequant_lora_f16": (DEQ + ("A_cat", "lda", "B", "nseg", "seg_rows", "scale", "stream"),
                                  dict(DEQ_BASE, A_cat=F, lda=64, B=F, nseg=1, seg_rows=16, scale=2.0)),
    "haff_gemm_nf4_f16": (NF4_GEMM + ("stream",), NF4_GEMM_BASE),
    "haff_gemm_nf4_lora_f16": (NF4_GEMM + ("t", "ldt", "B", "nseg", "seg_rows", "scale", "stream"),
                               dict(NF4_GEMM_BASE, t=F, ldt=8, B=F, nseg=1, seg_rows=16, scale=2.0)),
    "haff_int8_quantize_weight_f16": (("W", "ldw", "N", "K", "row_map", "CB", "SCB", "stream"),
                                      dict(W=F, ldw=64, N=4, K=64, row_map=None, CB=F, SCB=F, stream=None)),
    "haff_int8_quantize_act_f16": (("A", "lda", "M", "K", "threshold", "seg_rows", "seg_valid", "masks", "CA", "ldca", "SCA", "cols",
                                    "ncols", "stream"),
                                   dict(A=F, lda=64, M=1, K=64, threshold=6.0, seg_rows=1, seg_valid=None, masks=F, CA=F, ldca=64, SCA=F,
                                        cols=F, ncols=F, stream=None)),
    "haff_gemm_int8_f16": (("A", "lda", "CA", "ldca", "SCA", "CB", "SCB", "cols", "ncols", "seg_rows", "C", "ldc", "bias", "resid", "ldr",
                            "row_map", "M", "N", "K", "act", "out_f32", "swiglu", "form", "stream"),
                           dict(A=F, lda=64, CA=F, ldca=64, SCA=F, CB=F, SCB=F, cols=None, ncols=None, seg_rows=1, C=F, ldc=64, bias=None,
                                resid=None, ldr=0, row_map=None, M=1, N=64, K=64, act=0, out_f32=0, swiglu=0, form=0, stream=None)),
}

# the stored rows every NF4 dequantiser and the quantiser take: whole 64-blocks, both tables present and on their words
NF4_ROWS = [(dict(N=0), BAD), (dict(N=-1), BAD), (dict(K=0), BAD), (dict(packed=None), BAD), (dict(absmax=None), BAD),
            (dict(absmax=F + 2), BAD)]
# ... the output rows of the two row-major dequantisers (K = 100: was test_nf4_cpu.py, test_lora_serve_cpu.py)
DEQ_ROWS = NF4_ROWS + [(dict(K=100, ldo=100), BAD), (dict(K=96, ldo=96), BAD), (dict(ldo=60), BAD), (dict(ldo=56), BAD), (dict(ldo=68), BAD),
                       (dict(out=None), BAD), (dict(out=ODD), BAD), (dict(packed=F + 2), BAD),
                       (dict(K=96, ldo=96, out=ODD), BAD), (dict(N=0, packed=F + 2), BAD)]               # two rules at once
# the operands of an NF4 product. M > 64 is the -2 rule; with a zero dimension -1 still wins, with any other -1 rule -2 does
NF4_OPERANDS = [(dict(M=0), BAD), (dict(N=0), BAD), (dict(K=0), BAD), (dict(M=-1), BAD),
                (dict(M=65), UNS), (dict(M=129), UNS),                                                      # was: test_nf4_cpu.py
                (dict(K=96, lda=96), BAD), (dict(lda=60), BAD), (dict(lda=68), BAD), (dict(K=128, lda=64), BAD),
                (dict(A=None), BAD), (dict(Wq=None), BAD), (dict(absmax=None), BAD), (dict(C=None), BAD),
                (dict(A=ODD), BAD), (dict(Wq=F + 4), BAD), (dict(absmax=F + 2), BAD),
                (dict(swiglu=1, N=48, ldc=48, ldr=48), BAD), (dict(swiglu=1, resid=F), BAD),
                # two rules at once
                (dict(M=65, N=0), BAD), (dict(M=65, K=0), BAD),
                (dict(M=65, K=96, lda=96), UNS), (dict(M=65, K=96), UNS), (dict(M=65, A=None), UNS), (dict(M=65, Wq=F + 4), UNS),
                (dict(M=65, lda=60), UNS), (dict(M=65, swiglu=1, N=48), UNS), (dict(M=65, swiglu=1, resid=F), UNS),
                (dict(K=96, lda=96, A=ODD), BAD), (dict(A=ODD, swiglu=1, N=48), BAD)]
# the adapters' layout, shared by both LoRA entry points (was: test_lora_serve_cpu.py)
LORA_LAYOUT = [(dict(nseg=0), BAD), (dict(nseg=-1), BAD), (dict(seg_rows=0), BAD), (dict(seg_rows=-16), BAD), (dict(seg_rows=24), BAD),
               (dict(seg_rows=40), BAD), (dict(B=None), BAD), (dict(B=ODD), BAD), (dict(B=F + 4), BAD)]
# the operands both int8 quantisers and the product share
I8_K = [(dict(K=0), BAD), (dict(K=-64), BAD)]

CASES = {
    "haff_nf4_quantize_f16": NF4_ROWS + [
        (dict(K=96, ldw=96), BAD), (dict(ldw=60), BAD), (dict(double_quant=2), BAD), (dict(workspace_bytes=60), BAD),   # was: test_nf4_cpu.py
        (dict(W=ODD), BAD),                                                                                             # was: test_nf4_cpu.py
        (dict(ldw=56), BAD), (dict(ldw=68), BAD), (dict(double_quant=-1), BAD), (dict(W=None), BAD), (dict(offset=None), BAD),
        (dict(workspace=None), BAD), (dict(packed=F + 2), BAD), (dict(workspace=F + 2), BAD), (dict(workspace_bytes=0), BAD),
        (dict(N=64, K=128, ldw=128, workspace_bytes=508), BAD),                    # 4 * N * K / 64 = 512
        (dict(K=96, ldw=96, W=ODD), BAD), (dict(workspace_bytes=0, packed=F + 2), BAD), (dict(N=0, workspace=None), BAD)],
    "haff_nf4_dequant_f16": DEQ_ROWS,
    "haff_nf4_dequant_t_f16": NF4_ROWS + [           # was: test_qlora_cpu.py (all but the last two lines)
        (dict(K=100), BAD), (dict(ldo=8), BAD), (dict(N=13, ldo=13), BAD), (dict(N=13, ldo=8), BAD), (dict(out=ODD), BAD),
        (dict(packed=F + 4), BAD), (dict(row_map=F + 2), BAD), (dict(out=None), BAD),
        (dict(packed=ODD), BAD),                     # 16-byte code chunks: the row-major forms take this address
        (dict(N=17, ldo=16), BAD), (dict(ldo=20), BAD), (dict(K=96), BAD),
        (dict(K=100, out=ODD), BAD), (dict(ldo=8, row_map=F + 2), BAD)],                                    # two rules at once
    "haff_nf4_dequant_lora_f16": DEQ_ROWS + LORA_LAYOUT + [
        (dict(K=100, ldo=100, lda=100), BAD), (dict(nseg=5), BAD), (dict(A_cat=None), BAD), (dict(A_cat=ODD), BAD), (dict(lda=56), BAD),
        (dict(lda=68), BAD), (dict(K=128, ldo=128, lda=64), BAD),
        (dict(out=ODD, nseg=0), BAD), (dict(nseg=5, lda=56), BAD)],                                         # two rules at once
    "haff_gemm_nf4_f16": NF4_OPERANDS,
    "haff_gemm_nf4_lora_f16": NF4_OPERANDS + LORA_LAYOUT + [
        (dict(swiglu=1, N=48, ldc=48, ldr=48, nseg=2, ldt=16), BAD), (dict(swiglu=1, resid=F, nseg=2, ldt=16), BAD),
        (dict(nseg=5, ldt=40), BAD), (dict(t=None), BAD), (dict(t=ODD), BAD), (dict(nseg=3, ldt=16), BAD), (dict(ldt=12), BAD),
        (dict(nseg=0, ldt=0), BAD), (dict(ldt=0), BAD), (dict(nseg=2, ldt=8), BAD),
        # two rules at once: the product's own checks, -2 included, come before the adapters'
        (dict(M=65, nseg=0), UNS), (dict(M=65, t=None), UNS), (dict(M=65, B=ODD, ldt=12), UNS), (dict(M=0, nseg=0), BAD),
        (dict(A=ODD, t=ODD), BAD)],
    "haff_int8_quantize_weight_f16": I8_K + [
        (dict(K=96, ldw=96), BAD),                                                                          # was: test_int8_cpu.py
        (dict(N=0), BAD), (dict(N=-1), BAD), (dict(ldw=68), BAD), (dict(ldw=56), BAD), (dict(K=128, ldw=64), BAD),
        (dict(W=None), BAD), (dict(CB=None), BAD), (dict(SCB=None), BAD), (dict(W=ODD), BAD), (dict(CB=ODD), BAD), (dict(SCB=F + 2), BAD),
        (dict(K=96, ldw=96, CB=ODD), BAD), (dict(N=0, W=None), BAD)],                                       # two rules at once
    "haff_int8_quantize_act_f16": I8_K + [
        (dict(threshold=-1.0), BAD), (dict(masks=None), BAD),                                               # was: test_int8_cpu.py
        (dict(M=0), BAD), (dict(M=-1), BAD), (dict(K=96, lda=96, ldca=96), BAD), (dict(seg_rows=0), BAD), (dict(seg_rows=-1), BAD),
        (dict(lda=68), BAD), (dict(lda=56), BAD), (dict(ldca=72), BAD), (dict(ldca=48), BAD), (dict(K=128, lda=128, ldca=64), BAD),
        (dict(threshold=NAN), BAD), (dict(threshold=-0.5, masks=None), BAD), (dict(threshold=1e-30, masks=None), BAD),
        (dict(A=None), BAD), (dict(CA=None), BAD), (dict(SCA=None), BAD), (dict(cols=None), BAD), (dict(ncols=None), BAD),
        (dict(A=ODD), BAD), (dict(CA=ODD), BAD), (dict(SCA=F + 2), BAD), (dict(masks=F + 2), BAD),
        (dict(threshold=0.0, masks=F + 2), BAD),                                   # a mask that is not read still has to be aligned
        (dict(threshold=NAN, M=0), BAD), (dict(masks=None, A=ODD), BAD), (dict(K=96, lda=96, ldca=96, threshold=-1.0), BAD)],
    "haff_gemm_int8_f16": I8_K + [
        (dict(CA=F + 1), BAD), (dict(M=65, form=1), UNS),                                                   # was: test_int8_cpu.py
        (dict(M=129, form=1), UNS), (dict(M=0), BAD), (dict(N=0), BAD), (dict(M=-1), BAD), (dict(K=96, ldca=96), BAD),
        (dict(seg_rows=0), BAD), (dict(seg_rows=-1), BAD), (dict(form=-1), BAD), (dict(form=3), BAD),
        (dict(CA=None), BAD), (dict(SCA=None), BAD), (dict(CB=None), BAD), (dict(SCB=None), BAD), (dict(C=None), BAD),
        (dict(ldca=72), BAD), (dict(ldca=48), BAD), (dict(K=128, ldca=64), BAD),
        # the outlier columns come as a pair, and bring the f16 rows with them
        (dict(cols=F), BAD), (dict(ncols=F), BAD), (dict(cols=F, ncols=F, A=None), BAD), (dict(cols=F, ncols=F, lda=32), BAD),
        (dict(CA=ODD), BAD), (dict(CB=ODD), BAD), (dict(SCA=F + 2), BAD), (dict(SCB=F + 2), BAD),
        (dict(swiglu=1, N=48), BAD), (dict(swiglu=1, resid=F), BAD),
        # a -1 rule and the -2 rule at once: -1 is checked first
        (dict(M=65, form=1, K=96, ldca=96), BAD), (dict(M=65, form=1, CB=ODD), BAD), (dict(M=65, form=1, swiglu=1, N=48), BAD),
        (dict(M=65, form=1, cols=F), BAD), (dict(M=65, form=1, seg_rows=0), BAD), (dict(M=65, form=1, C=None), BAD),
        (dict(M=65, form=3), BAD), (dict(K=96, ldca=96, CA=ODD, swiglu=1, resid=F), BAD)],
}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(haff.LIB_PATH):
        haff.build_library()
    return haff.load_library()


@pytest.mark.parametrize("name", list(ENTRY))
def test_refusals_and_their_codes(lib, name):
    order, base = ENTRY[name]
    assert all(want in (BAD, UNS) for _, want in CASES[name])      # nothing here may get as far as a launch
    wrong = []
    for over, want in CASES[name]:
        assert set(over) <= set(base), (name, over)
        args = dict(base, **over)
        got = int(getattr(lib, name)(*[args[k] for k in order]))
        if got != want:
            wrong.append((over, got, want))
    assert not wrong, wrong


@pytest.mark.parametrize("name", list(ENTRY))
def test_every_checked_pointer_has_a_null_and_a_misaligned_case(name):
    """The pointers each entry point checks, by name: every one has a case of its own that spoils only it (null where null is
    refused, off its alignment where that is). A pointer listed in neither tuple is passed through unchecked."""
    null, misaligned = {
        "haff_nf4_quantize_f16": (("W", "packed", "absmax", "offset", "workspace"), ("W", "packed", "absmax", "workspace")),
        "haff_nf4_dequant_f16": (("packed", "absmax", "out"), ("packed", "absmax", "out")),
        "haff_nf4_dequant_t_f16": (("packed", "absmax", "out"), ("packed", "absmax", "out", "row_map")),
        "haff_nf4_dequant_lora_f16": (("packed", "absmax", "out", "A_cat", "B"), ("packed", "absmax", "out", "A_cat", "B")),
        "haff_gemm_nf4_f16": (("A", "Wq", "absmax", "C"), ("A", "Wq", "absmax")),
        "haff_gemm_nf4_lora_f16": (("A", "Wq", "absmax", "C", "t", "B"), ("A", "Wq", "absmax", "t", "B")),
        "haff_int8_quantize_weight_f16": (("W", "CB", "SCB"), ("W", "CB", "SCB")),
        "haff_int8_quantize_act_f16": (("A", "masks", "CA", "SCA", "cols", "ncols"), ("A", "masks", "CA", "SCA")),
        "haff_gemm_int8_f16": (("CA", "SCA", "CB", "SCB", "C"), ("CA", "SCA", "CB", "SCB")),
    }[name]
    alone = [over for over, _ in CASES[name] if len(over) == 1]
    for ptr in null:
        assert {ptr: None} in alone, (name, ptr)
    for ptr in misaligned:
        assert any(list(over) == [ptr] and over[ptr] is not None and over[ptr] != F for over in alone), (name, ptr)


def test_every_quantised_entry_point_is_covered():
    exported = {n for n in haff.EXPORTED_SYMBOLS if "nf4" in n or "int8" in n}
    assert set(ENTRY) == set(CASES) == exported, set(ENTRY) ^ exported
