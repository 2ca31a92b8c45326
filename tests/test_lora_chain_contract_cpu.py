"""The host-side contract of the LoRA, TN GEMM and decode-chain family (no GPU): which inputs the 22 code-returning entry points of lora.hip,
gemm_tn.hip and decode_chain.hip refuse, and with WHICH code: -1 (bad argument) or -2 (a shape the kernels do not serve). The order of the
checks is part of the contract: an input that breaks a -1 rule and a -2 rule at once gets the code of the rule checked first. Every call
below is refused before anything is launched; the device addresses are fake, 16-byte aligned unless a case says otherwise, and never
dereferenced; `layers` of haff_decode_chain_bf16 is read on the HOST and is a real ctypes array of haff_chain_layer holding fake addresses.
A pointer whose alignment no rule looks at (t^T of the q|k|v forward, dt^T and A of dx, the workspace and out of haff_lora_tn, the f32 tables
of the chain) and an ADMISSIBLE absent mask have no case of their own, since such a call goes on to launch: the mask tables pair every
subset with K = 64, so an admissible subset shows as the -2 of the K % 128 rule, which is judged after the mask rule.
The expected codes and the four count-returning functions' values were recorded from the library as it stood before the three files' host
halves were reorganised around one argument setup, one grid rule, one mask rule and one chain geometry (built from the parent commit and
loaded through HAFF_LIB_PATH); they are not derived from the code under test."""
import ctypes
import os

import pytest

import haff

F = 0x10000         # 16-byte aligned, never dereferenced
BAD, UNS = -1, -2


def entry(order, **base):
    order = order.split()
    base = dict({k: (None if k == "stream" else F) for k in order}, **base)
    assert set(base) == set(order), set(base) ^ set(order)
    return order, base


def each(key, *values, want=BAD, **also):
    return [(dict({key: v}, **also), want) for v in values]


def nulls(*keys, want=BAD, **also):
    return [(dict({k: None}, **also), want) for k in keys]


def off(*keys, by=(2, 8), want=BAD, **also):
    return [(dict({k: F + b}, **also), want) for k in keys for b in by]


class ChainLayer(ctypes.Structure):
    _fields_ = [(n, ctypes.c_void_p) for n in ("wqkv", "wo", "wgu", "wd", "kcache", "vcache")]


_KEEP = []          # the layer tables stay alive for the whole module


def layers(n, at=None, member=None, value=None):
    """The address of a host array of n haff_chain_layer with fake device addresses; layer `at` gets `member` = value."""
    arr = (ChainLayer * n)(*[ChainLayer(*[F + 0x1000 * (6 * i + j) for j in range(6)]) for i in range(n)])
    if at is not None:
        setattr(arr[at], member, value)
    _KEEP.append(arr)
    return ctypes.addressof(arr)


MEMBERS = ("wqkv", "wo", "wgu", "wd", "kcache", "vcache")

QKV = dict(ld_qkv=768, ldt=32, ldb=8, ldo=256, M=20, H=256, d=128, T=5, scale=2.0)
QKV_ORDER = "qkv ld_qkv tT ldt Bq Bv ldb cos_sin q_out k_out v_out ldo M H d T scale stream"
QKV3_ORDER = QKV_ORDER.replace("Bv ldb", "Bv Bk ldb")
QKV_PTRS = ("qkv", "Bq", "Bv", "cos_sin", "q_out", "k_out", "v_out")          # t^T has no alignment rule
QKV_CASES = (nulls("tT", *QKV_PTRS) + each("M", 0, -1) + each("T", 0) + each("H", 0) + each("d", 0, 64, 256, want=UNS)
             + each("H", 192, 64, want=UNS) + each("ldb", 0, 7, 9, 16, want=UNS)
             + each("ld_qkv", 760, 767, 772) + each("ldo", 248, 255, 260) + each("ldt", 19, 0) + off(*QKV_PTRS)
             # a -2 rule with a -1 rule judged earlier, and with one judged later
             + each("d", 64, M=0) + each("H", 192, qkv=None) + each("ldb", 16, T=0)
             + each("d", 64, want=UNS, ldo=248) + each("H", 192, want=UNS, ld_qkv=772) + each("ldb", 16, want=UNS, q_out=F + 2)
             + each("d", 64, want=UNS, ldt=19))
# the k adapter's B: null or misaligned is judged BEFORE the -2 rules, the other operands' alignment after them
QKV3_CASES = QKV_CASES + nulls("Bk") + off("Bk") + nulls("Bk", d=64) + off("Bk", d=64) + off("Bq", want=UNS, d=64)

RBWD = dict(ld_in=256, ld_out=768, M=20, H=256, d=128, T=5)
RBWD_PTRS = ("dq", "dk", "dv", "cos_sin", "dqkv")
RBWD_CASES = (nulls(*RBWD_PTRS) + each("M", 0, -1) + each("T", 0) + each("H", 0) + each("d", 0, 64, want=UNS) + each("H", 192, want=UNS)
              + each("ld_in", 248, 255, 260) + each("ld_out", 760, 767, 772) + off(*RBWD_PTRS)
              + each("d", 64, M=0) + each("H", 192, dqkv=None) + each("d", 64, want=UNS, ld_in=248) + each("H", 192, want=UNS, dq=F + 8))

DX = dict(ldt=32, lda=256, ldk=256, ldx=256, accumulate=1, M=20, K=256, scale=2.0)
DX_CASES = (nulls("dtT", "dx") + each("M", 0, -1) + each("K", 0, -128) + each("K", 64, 200, 257, want=UNS) + each("ldt", 19, 0)
            + each("lda", 255, 128) + each("ldx", 248, 255, 260) + off("dx")
            + each("K", 64, M=0) + each("K", 64, dx=None) + each("K", 64, want=UNS, ldx=56) + each("K", 64, want=UNS, dx=F + 2)
            + each("K", 64, want=UNS, ldt=19))
DX_MASK_LD = each("ldk", 248, 255, 260)       # judged only where a mask is given: every base below gives at least keep / keep_q


def dx_masks(names, admissible):
    """Every subset of the entry point's masks at K = 64: -2 (the K % 128 rule, judged later) for an admissible one, else -1; and
    each mask of the full set off its boundary, at K = 256 (-1) and at K = 64 (keep_k: -1, judged before K % 128; the others: -2)."""
    cases = []
    for bits in range(1 << len(names)):
        have = tuple(n for i, n in enumerate(names) if bits >> i & 1)
        over = {n: (F if n in have else None) for n in names}
        cases.append((dict(over, K=64), UNS if have in admissible else BAD))
        if have not in admissible:
            cases.append((over, BAD))
    for n in names:
        cases += off(n) + off(n, K=64, want=BAD if n == "keep_k" else UNS)
    return cases


DX1_CASES = DX_CASES + nulls("A2") + DX_MASK_LD + dx_masks(("keep",), ((), ("keep",)))
DX2_CASES = DX_CASES + nulls("A2") + DX_MASK_LD + dx_masks(("keep_q", "keep_v"), (("keep_q", "keep_v"),))
DX3_CASES = (DX_CASES + nulls("A3") + DX_MASK_LD
             + dx_masks(("keep_q", "keep_v", "keep_k"), ((), ("keep_q",), ("keep_q", "keep_v", "keep_k")))
             # the seven ordering facts, by name: keep_k's alignment before the K % 128 rule, keep_q's and keep_v's after it
             + [(dict(K=64, keep_k=F + 2), BAD), (dict(K=64, keep_q=F + 2), UNS), (dict(K=64, keep_v=F + 2), UNS)])

TN = dict(lds=32, R=8, ldb=130, M=20, N=130, workspace_elems=1040, ldo=130, out_f32=0, transposed=0, j_valid=8, scale=1.0)
TN_CASES = (nulls("sT", "big", "workspace", "out") + each("M", 0, -1) + each("N", 0) + each("j_valid", 0, -1, 9) + each("R", 0, 16)
            + each("R", 4, 12, want=UNS, j_valid=4) + each("R", 24, 32, want=UNS)
            + each("lds", 16, 24, 31, 36) + each("ldb", 128, 129, 131) + each("N", 129, ldb=132, ldo=132) + off("sT") + off("big", by=(1, 2))
            + each("workspace_elems", 1039, 0) + each("ldo", 129, 0) + each("ldo", 7, transposed=1) + each("ldo", 4, transposed=1, j_valid=5)
            # ordering: j_valid > R before the rank rule, the rank rule before the stride, workspace and ldo rules
            + [(dict(R=4, j_valid=5), BAD), (dict(R=4, j_valid=4, lds=12), UNS), (dict(R=4, j_valid=4, M=0), BAD),
               (dict(R=4, j_valid=4, out=None), BAD), (dict(R=4, j_valid=4, workspace_elems=0), UNS), (dict(R=4, j_valid=4, sT=F + 2), UNS),
               (dict(R=4, j_valid=4, ldo=0), UNS)])

OUT = dict(ldt=20, ldy=64, M=20, N=64, scale=2.0)
OUT_CASES = (nulls("tT", "B", "y") + each("M", 0, -1) + each("N", 0) + each("N", 60, 4, 65, want=UNS) + each("ldt", 16, 19, 22)
             + each("ldt", 21, M=21) + each("ldy", 56, 63, 68) + off("tT", by=(2, 4)) + off("B", "y")
             + each("N", 60, M=0) + each("N", 60, y=None) + each("N", 60, want=UNS, ldy=56) + each("N", 60, want=UNS, tT=F + 2)
             + each("N", 60, want=UNS, ldt=16))

GU = dict(ldt=20, ldg=128, ldy=64, M=20, F=64, scale=2.0)
GU_CASES = (nulls("tT", "Bg", "Bu", "gu", "y") + each("M", 0, -1) + each("F", 0) + each("F", 56, 8, 72, want=UNS) + each("ldt", 16, 19, 22)
            + each("ldg", 120, 127, 132) + each("ldy", 56, 63, 68) + off("tT", by=(2, 4)) + off("Bg", "Bu", "gu", "y")
            + each("F", 56, M=0) + each("F", 56, gu=None) + each("F", 56, want=UNS, ldg=104) + each("F", 56, want=UNS, y=F + 8)
            + each("F", 56, want=UNS, tT=F + 4))

GTN = dict(lda=64, ldb=64, M=300, N1=64, N2=64, workspace_elems=8192, out_f32=0)
GTN_CASES = (nulls("A", "B", "workspace", "out") + each("M", 0, -1) + each("N1", 0) + each("N2", 0) + each("lda", 56, 63) + each("ldb", 56, 63)
             + each("lda", 68, 65, want=UNS) + each("ldb", 68, 65, want=UNS) + each("N1", 60, 4, want=UNS) + each("N2", 60, 4, want=UNS)
             + off("A", "B", "out", want=UNS) + off("workspace", by=(2, 4, 8)) + each("workspace_elems", 8191, 4096, 0)
             # ordering: a misaligned operand is -2 ("the caller transposes"); the workspace's alignment is judged before that rule and
             # its size after it
             + [(dict(A=F + 2), UNS), (dict(workspace=F + 8), BAD), (dict(workspace=F + 8, N1=60), BAD),
                (dict(workspace_elems=4096, out=F + 2), UNS), (dict(N1=60, M=0), BAD), (dict(N1=60, B=None), BAD),
                (dict(N1=60, workspace_elems=0), UNS), (dict(lda=68, ldb=56), BAD)])

CHAIN = dict(layers=layers(2), n_layers=2, M=2, hidden=256, ffn=256, heads=2, eps=1e-5, tmax=16, scale=0.088, per_stage_launches=0)
CHAIN_PTRS = ("x", "qkv", "att", "g", "ssq_a", "ssq_b", "ws")                  # the ones whose alignment is judged
CHAIN_UNS = (dict(hidden=128, heads=1), dict(hidden=384, heads=3), dict(hidden=8448, heads=66), dict(heads=3), dict(hidden=512), dict(ffn=384),
             dict(hidden=0, heads=0), dict(ffn=0))
CHAIN_CASES = (
    nulls("layers", *CHAIN_PTRS, "stats0", "cos_sin", "nk_rows", "sync") + off(*CHAIN_PTRS) + each("n_layers", 0, -1)
    + each("n_layers", 49, layers=layers(49)) + each("M", 0, 9) + each("tmax", 0, -1) + [(g, UNS) for g in CHAIN_UNS]
    # a null or a misaligned member of layer 0 and of the last layer (the host loop reaches every layer)
    + [(dict(layers=layers(2, at, m, v)), BAD) for at in (0, 1) for m in MEMBERS for v in (None, F + 2, F + 8)]
    + [(dict(layers=layers(48, 47, m, v), n_layers=48), BAD) for m in ("wqkv", "vcache") for v in (None, F + 8)]
    # the geometry's -2 is judged after layers / n_layers / M and before every other pointer, tmax and the layers' members
    + [(dict(g, **e), BAD) for g in CHAIN_UNS[:2] + CHAIN_UNS[5:6] for e in (dict(layers=None), dict(n_layers=0), dict(n_layers=49), dict(M=9))]
    + [(dict(g, **l), UNS) for g in CHAIN_UNS[:2] + CHAIN_UNS[5:6]
       for l in (dict(ws=None), dict(ws=F + 8), dict(x=None), dict(tmax=0), dict(layers=layers(2, 0, "wo", None)), dict(layers=layers(2, 1, "kcache", F + 2)))])

ENTRY = {
    # ---- lora.hip
    "haff_lora_qkv_rope_fwd": entry(QKV_ORDER, **QKV),
    "haff_lora_qkv3_rope_fwd": entry(QKV3_ORDER, **QKV),
    "haff_lora_qkv_rope_bwd": entry("dq dk dv ld_in cos_sin dqkv ld_out M H d T stream", **RBWD),
    "haff_lora_dx": entry("dtT ldt A2 lda keep ldk dx ldx accumulate M K scale stream", **DX),
    "haff_lora_dx2": entry("dtT ldt A2 lda keep_q keep_v ldk dx ldx accumulate M K scale stream", **DX),
    "haff_lora_dx3": entry("dtT ldt A3 lda keep_q keep_v keep_k ldk dx ldx accumulate M K scale stream", **DX),
    "haff_lora_tn": entry("sT lds R big ldb M N workspace workspace_elems out ldo out_f32 transposed j_valid scale stream", **TN),
    "haff_lora_out": entry("tT ldt B y ldy M N scale stream", **OUT),
    "haff_lora_gu_swiglu": entry("tT ldt Bg Bu gu ldg y ldy M F scale stream", **GU),
    # ---- gemm_tn.hip
    "haff_gemm_tn_bf16": entry("A lda B ldb M N1 N2 workspace workspace_elems out out_f32 stream", **GTN),
    # ---- decode_chain.hip
    "haff_decode_chain_bf16": entry("layers n_layers M hidden ffn heads x qkv att g ssq_a ssq_b ws stats0 eps cos_sin nk_rows tmax scale sync "
                                    "per_stage_launches stream", **CHAIN),
    "haff_decode_chain_status": entry("sync n_layers stream", n_layers=2),
}
CASES = {
    "haff_lora_qkv_rope_fwd": QKV_CASES, "haff_lora_qkv3_rope_fwd": QKV3_CASES, "haff_lora_qkv_rope_bwd": RBWD_CASES,
    "haff_lora_dx": DX1_CASES, "haff_lora_dx2": DX2_CASES, "haff_lora_dx3": DX3_CASES, "haff_lora_tn": TN_CASES,
    "haff_lora_out": OUT_CASES, "haff_lora_gu_swiglu": GU_CASES, "haff_gemm_tn_bf16": GTN_CASES,
    "haff_decode_chain_bf16": CHAIN_CASES,
    "haff_decode_chain_status": nulls("sync") + each("n_layers", 0, -1, 49),
}
# the fp16 instances: same arguments, same contract
for _name in [n for n in ENTRY if not n.startswith("haff_decode_chain")]:
    _f16 = _name.replace("_bf16", "_f16") if _name.endswith("_bf16") else _name + "_f16"
    ENTRY[_f16], CASES[_f16] = ENTRY[_name], CASES[_name]

NO_UNS = ("haff_decode_chain_status",)

# ---- the four count-returning functions (pure host arithmetic)
# haff_lora_tn_workspace_elems(M, R, N): row blocks of lora_tn_rows_per_block(M) rows (a multiple of 64, ~16 blocks) x R x N
LORA_TN_WS = {(1, 8, 130): 1040, (1024, 8, 130): 16640, (1025, 8, 130): 9360, (1025, 16, 130): 18720, (2048, 16, 130): 33280,
              (2049, 16, 130): 22880, (3072, 8, 2): 256, (3073, 8, 2): 208, (0, 8, 130): -1, (20, 0, 130): -1, (20, 8, 0): -1, (-5, 8, 130): -1,
              (20, 16, 130): 2080, (1 << 20, 16, 1 << 23): -2, (1 << 20, 16, 8388607): 2147483392}
# haff_gemm_tn_workspace_elems(M, N1, N2): splits x N1 x N2, splits = ceil(M / rows_per_split), at most 64 and at least 256 rows each
GEMM_TN_WS = {(256, 64, 64): 4096, (257, 64, 64): 8192, (16384, 64, 64): 262144, (16385, 64, 64): 212992, (20480, 64, 64): 262144,
              (1 << 20, 128, 128): 1048576, (65536, 256, 256): 4194304, (65536, 256, 512): 8388608, (65536, 512, 512): 8388608,
              (65536, 2048, 2048): 8388608, (65536, 8192, 8192): 67108864, (256, 65536, 65536): -2, (1, 8, 8): 64, (1000, 1024, 1024): 4194304, (4096, 1024, 1024): 8388608, (4097, 1024, 1024): 8388608, (0, 64, 64): -1,
              (256, 0, 64): -1, (256, 64, -8): -1}
# haff_decode_chain_supported(M, hidden, ffn, heads, n_layers): workgroups per layer, 0 for a refused geometry
CHAIN_SUPPORTED = {(1, 256, 256, 2, 1): 130, (2, 256, 256, 2, 1): 132, (3, 256, 256, 2, 1): 134, (4, 256, 256, 2, 1): 136,
                   (5, 256, 256, 2, 1): 138, (6, 256, 256, 2, 1): 140, (7, 256, 256, 2, 1): 142, (8, 256, 256, 2, 1): 144,
                   (0, 256, 256, 2, 1): 0, (9, 256, 256, 2, 1): 0, (1, 256, 256, 2, 0): 0, (1, 256, 256, 2, 49): 0, (1, 256, 256, 2, 48): 130,
                   (1, 128, 256, 1, 1): 0, (1, 384, 256, 3, 1): 0, (1, 256, 384, 2, 1): 0, (1, 256, 256, 3, 1): 0, (1, 8448, 256, 66, 1): 0,
                   (1, 8192, 256, 64, 1): 3664, (1, 4096, 11008, 32, 32): 2512, (8, 5120, 13824, 40, 40): 3424}
# haff_decode_chain_sync_words(n_layers, hidden): Llama 7B and 13B widths, and the refusals' 0
CHAIN_SYNC_WORDS = {(1, 256): 2624, (32, 4096): 98336, (40, 5120): 128032, (48, 5120): 153632, (0, 4096): 0, (49, 4096): 0, (32, 0): 0}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(haff.LIB_PATH):
        haff.build_library()
    return haff.load_library()


def test_every_code_returning_entry_point_of_the_three_files_has_cases():
    assert len(ENTRY) == 22 and set(CASES) == set(ENTRY)       # the other four return counts: the value tables below


@pytest.mark.parametrize("name", sorted(CASES))
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


def test_the_minus_two_code_is_recorded_where_an_entry_point_has_one():
    for name, cases in CASES.items():
        assert {want for _, want in cases} == ({BAD} if name in NO_UNS else {BAD, UNS}), name


@pytest.mark.parametrize("fn,table", (("haff_lora_tn_workspace_elems", LORA_TN_WS), ("haff_gemm_tn_workspace_elems", GEMM_TN_WS),
                                      ("haff_decode_chain_supported", CHAIN_SUPPORTED), ("haff_decode_chain_sync_words", CHAIN_SYNC_WORDS)),
                         ids=lambda v: v if isinstance(v, str) else "")
def test_counts(lib, fn, table):
    got = {args: int(getattr(lib, fn)(*args)) for args in table}
    assert got == table
