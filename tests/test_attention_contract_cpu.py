"""The attention family's host-side contract (no GPU): which inputs each entry point refuses, and with WHICH code — -1 (bad argument)
or -2 (a geometry the kernels do not serve). The order of the checks is part of the contract: an input that breaks a -1 rule and a
-2 rule at once gets the code of the rule checked first. Every case below is refused before anything is launched (the addresses are
fake and never dereferenced); no case would pass validation. The expected codes were recorded from the library as it stood before the
host halves of attention.hip, attention_f32.hip, attention_bwd.hip and window_attention.hip were reorganised around named argument
setup and one operand contract; they are not derived from the code under test."""
import os

import pytest

import haff

F = 0x10000         # 16-byte aligned, never dereferenced
ODD = F + 8         # 8-byte aligned only
BAD, UNS = -1, -2

QKVO = tuple(f"{x}{s}" for x in "qkvo" for s in ("", "_sb", "_sh", "_st"))
ROWS = tuple(n for n in QKVO if n not in ("q_st", "o_st"))      # decode: one query row, no token stride for q and the output
# [B][H][N][d] planes, N = 196, d = 80, H = 2
PLANES = dict(q=F, k=F, v=F, o=F, **{f"{x}_sb": 31360 for x in "qkvo"}, **{f"{x}_sh": 15680 for x in "qkvo"},
              **{f"{x}_st": 80 for x in "qkvo"})


def fused(n, hd=160, k_off=1, v_off=2):
    """q | k | v rows of one fused projection ([B][n][3 * hd] 16-bit), the output token-major [B][n][hd]"""
    return dict(q=F, k=F + 2 * hd * k_off, v=F + 2 * hd * v_off, o=F, q_sb=3 * hd * n, k_sb=3 * hd * n, v_sb=3 * hd * n, o_sb=hd * n,
                q_sh=80, k_sh=80, v_sh=80, o_sh=80, q_st=3 * hd, k_st=3 * hd, v_st=3 * hd, o_st=hd)


REL = dict(relh=F, relw=F, S=14)
ATT_BASE = dict(PLANES, B=1, H=2, Nq=196, Nk=196, d=80, scale=0.1, causal=0, q_pos0=0, relh=None, relw=None, S=0, stream=None)
DEC_BASE = dict(q=F, q_sb=256, q_sh=128, k=F, k_sb=76800, k_sh=38400, k_st=128, v=F, v_sb=76800, v_sh=38400, v_st=128, o=F, o_sb=256,
                o_sh=128, B=1, H=2, Nk=300, d=128, scale=0.1, nk_rows=F, stream=None)
BWD_NEED = 128 + 2 * 64 * 128   # delta [B*H*Nq], then B*H*128*roundup(Nq, 64) dq sums
BWD_PTRS = ("q", "k", "v", "o", "dout", "dq", "dk", "dv")

# entry point (without its dtype suffix) -> (argument order, a base argument set that every case below spoils, its dtypes)
ENTRY = {
    "haff_attention": (QKVO + ("B", "H", "Nq", "Nk", "d", "scale", "causal", "q_pos0", "relh", "relw", "S", "stream"), ATT_BASE,
                       ("bf16", "f16", "f32")),
    "haff_attention_lse": (QKVO + ("B", "H", "Nq", "Nk", "d", "scale", "causal", "q_pos0", "lse", "stream"),
                           dict(PLANES, B=1, H=2, Nq=196, Nk=196, d=80, scale=0.1, causal=0, q_pos0=0, lse=F, stream=None), ("bf16", "f16")),
    "haff_global_attention": (QKVO + ("B", "H", "S", "d", "scale", "tab_h", "tab_w", "stream"),
                              dict(fused(4096), B=1, H=2, S=64, d=80, scale=0.1, tab_h=F, tab_w=F, stream=None), ("bf16", "f16")),
    "haff_attention_decode_rows": (ROWS + ("B", "H", "Nk", "d", "scale", "nk_rows", "stream"), DEC_BASE, ("bf16", "f16", "f32")),
    "haff_decode_attention_rope_rows": (("qkv", "ld", "kcache", "vcache", "cos_sin", "out", "B", "H", "d", "Tmax", "scale", "nk_rows", "stream"),
                                        dict(qkv=F, ld=768, kcache=F, vcache=F, cos_sin=F, out=F, B=1, H=2, d=128, Tmax=32, scale=0.1,
                                             nk_rows=F, stream=None), ("bf16", "f16")),
    "haff_relpos_tables": (("q", "q_sb", "q_sh", "q_st", "tab_h", "tab_w", "relh", "relw", "B", "H", "S", "d", "dtype", "stream"),
                           dict(q=F, q_sb=31360, q_sh=15680, q_st=80, tab_h=F, tab_w=F, relh=F, relw=F, B=1, H=2, S=14, d=80, dtype=0,
                                stream=None), ("",)),
    "haff_relpos_tables_bf16": (("q", "q_sb", "q_sh", "q_st", "tab_h", "tab_w", "relh", "relw", "B", "H", "S", "d", "stream"),
                                dict(q=F, q_sb=31360, q_sh=15680, q_st=80, tab_h=F, tab_w=F, relh=F, relw=F, B=1, H=2, S=14, d=80,
                                     stream=None), ("",)),
    "haff_window_attention": (QKVO + ("n_windows", "H", "S", "d", "scale", "tab_h", "tab_w", "grid_h", "grid_w", "pad_token", "stream"),
                              dict(fused(196), n_windows=25, H=2, S=14, d=80, scale=0.1, tab_h=F, tab_w=F, grid_h=0, grid_w=0, pad_token=0,
                                   stream=None), ("bf16", "f16")),
    "haff_attention_bwd": (("q", "k", "v", "o", "dout", "lse", "dq", "dk", "dv", "workspace", "workspace_elems", "ld", "B", "H", "Nq", "Nk",
                            "d", "scale", "causal", "q_pos0", "stream"),
                           dict({x: F for x in BWD_PTRS}, lse=F, workspace=F, workspace_elems=BWD_NEED, ld=256, B=1, H=2, Nq=64, Nk=64,
                                d=128, scale=0.1, causal=0, q_pos0=0, stream=None), ("bf16", "f16")),
}

ZERO_DIMS = [(dict(B=0), BAD), (dict(H=0), BAD), (dict(Nq=0), BAD), (dict(Nk=0), BAD), (dict(d=0), BAD), (dict(B=-1), BAD)]
# the twelve-term stride rule of the 16-bit family: q / k / v strides in whole 16-byte chunks, output strides in whole 8-byte ones
STRIDES16 = ([(dict({f"{x}_{s}": 84}), BAD) for x in "qkv" for s in ("sb", "sh", "st")] +
             [(dict({f"o_{s}": 82}), BAD) for s in ("sb", "sh", "st")] + [(dict(q_st=1028), BAD), (dict(q_sb=84, o_st=82, v_sh=84), BAD)])
# ... and of the f32 family: every stride in whole 16-byte chunks
STRIDES32 = [(dict({f"{x}_{s}": 82}), BAD) for x in "qkvo" for s in ("sb", "sh", "st")]
BIG = dict(S=40, Nk=160)        # a key grid no rel-pos kernel serves: not 64 wide, wider than the 32 the LDS tables hold
ATT16 = ZERO_DIMS + STRIDES16 + [
    (dict(d=136), BAD), (dict(d=68), BAD), (dict(d=-8), BAD),
    (dict(REL, causal=1), BAD), (dict(REL, S=0), BAD), (dict(REL, S=-14), BAD), (dict(REL, S=15), BAD),
    (dict(REL, **BIG), UNS), (dict(REL, S=33, Nk=66), UNS), (dict(REL, S=48, Nk=96), UNS), (dict(REL, d=128, **BIG), UNS),
    # a -1 rule and a -2 rule at once: -1 is checked first
    (dict(REL, causal=1, **BIG), BAD), (dict(REL, d=136, **BIG), BAD), (dict(REL, q_st=1028, **BIG), BAD), (dict(REL, B=0, **BIG), BAD)]
# fp16: the rel-pos instances stop at d <= 96. (In bf16 these launch, so they are cases of the f16 entry point only.)
ATT_F16 = [(dict(REL, d=128), UNS), (dict(REL, d=104), UNS), (dict(REL, d=128, S=64, Nk=4096), UNS),
           (dict(REL, d=128, causal=1), BAD), (dict(REL, d=128, S=15), BAD), (dict(REL, d=104, k_st=84), BAD)]
NK_BIG = dict(Nk=20000)         # the f32 kernel holds a score row per query in LDS: past 150 KB it is refused
ATT32 = ZERO_DIMS + STRIDES32 + [
    (dict(d=260), BAD), (dict(d=2), BAD), (dict(d=82), BAD), (dict(REL, S=0), BAD), (dict(REL, S=15), BAD), (dict(REL, S=0, causal=1), BAD),
    (NK_BIG, UNS), (dict(Nk=20000, causal=1, q_pos0=5), UNS), (dict(REL, S=20, Nk=20000), UNS),
    (dict(Nk=20000, d=260), BAD), (dict(REL, S=7, Nk=20000), BAD), (dict(Nk=20000, q_st=82), BAD), (dict(Nk=20000, H=0), BAD)]

DEC_DIMS = [(dict(nk_rows=None), BAD), (dict(B=0), BAD), (dict(H=0), BAD), (dict(Nk=0), BAD), (dict(d=0), BAD)]
DEC16 = DEC_DIMS + [(dict(d=136), BAD), (dict(d=68), BAD), (dict(q_sb=260), BAD), (dict(q_sh=132), BAD), (dict(k_sb=76804), BAD),
                    (dict(k_sh=38404), BAD), (dict(k_st=132), BAD), (dict(v_sb=76804), BAD), (dict(v_sh=38404), BAD), (dict(v_st=132), BAD),
                    (dict(o_sb=258), BAD), (dict(o_sh=130), BAD), (dict(nk_rows=None, d=136), BAD), (dict(nk_rows=None, B=0, o_sh=130), BAD)]
DEC32 = DEC_DIMS + [(dict(d=260), BAD), (dict(d=2), BAD), (dict(q_sb=258), BAD), (dict(q_sh=130), BAD), (dict(k_st=130), BAD),
                    (dict(v_sb=76802), BAD), (dict(o_sb=258), BAD), (dict(o_sh=130), BAD),
                    (dict(Nk=20000), UNS), (dict(Nk=40000, d=64), UNS),
                    (dict(Nk=20000, d=260), BAD), (dict(Nk=20000, nk_rows=None), BAD), (dict(Nk=20000, k_st=130), BAD)]

WIDE = dict(q_st=1 << 24, k_st=1 << 24, v_st=1 << 24)
PADDED = dict(grid_h=64, grid_w=64, pad_token=25 * 196)     # 5 x 5 windows of 14 over a 64 x 64 token grid, the pad row behind them
FAR_V = dict(v=F + (1 << 31))   # v 2 GiB behind k: an item still spans under 4 GiB, the V pad row of a padded grid may not

CASES = {
    "haff_attention_bf16": ATT16,
    "haff_attention_f16": ATT16 + ATT_F16,
    "haff_attention_f32": ATT32,
    "haff_attention_lse": ZERO_DIMS + STRIDES16 + [
        (dict(d=136), BAD), (dict(d=68), BAD), (dict(q=None), BAD), (dict(k=None), BAD), (dict(v=None), BAD), (dict(o=None), BAD),
        (dict(lse=None), BAD), (dict(q=ODD), BAD), (dict(k=ODD), BAD), (dict(v=ODD), BAD), (dict(o=F + 4), BAD), (dict(lse=F + 2), BAD),
        (dict(causal=1, q_pos0=-1), BAD), (dict(q=None, d=136), BAD), (dict(lse=F + 2, q_st=1028, causal=1, q_pos0=-1), BAD)],
    "haff_global_attention": [
        (dict(B=0), BAD), (dict(H=0), BAD), (dict(S=0), BAD), (dict(d=0), BAD), (dict(tab_h=None), BAD), (dict(tab_w=None), BAD),
        (dict(q_st=484), BAD), (dict(k_sh=84), BAD), (dict(v_sb=484), BAD), (dict(o_st=162), BAD), (dict(o_sb=82), BAD),
        (dict(S=32), UNS), (dict(S=14), UNS), (dict(d=64), UNS), (dict(d=84), UNS), (dict(k=F + 640, v=F + 320), UNS), (dict(v_st=488), UNS),
        (dict(v_sb=488), UNS), (dict(v_sh=88), UNS), (dict(q=ODD), UNS), (dict(k=F + 328), UNS), (dict(v=F + 648), UNS), (dict(tab_h=ODD), UNS),
        (dict(tab_w=ODD), UNS), (dict(q_st=1 << 19, k_st=1 << 19, v_st=1 << 19), UNS),
        # a -1 rule and a -2 rule at once: -1 is checked first
        (dict(S=32, tab_h=None), BAD), (dict(d=64, q_st=484), BAD), (dict(q=ODD, H=0), BAD), (dict(tab_w=ODD, o_st=162), BAD)],
    "haff_attention_decode_rows_bf16": DEC16,
    "haff_attention_decode_rows_f16": DEC16,
    "haff_attention_decode_rows_f32": DEC32,
    "haff_decode_attention_rope_rows": [
        (dict(B=0), BAD), (dict(H=0), BAD), (dict(d=0), BAD), (dict(d=64), BAD), (dict(d=256), BAD), (dict(Tmax=0), BAD),
        (dict(nk_rows=None), BAD), (dict(cos_sin=None), BAD), (dict(ld=772), BAD), (dict(qkv=ODD), BAD), (dict(kcache=ODD), BAD),
        (dict(vcache=ODD), BAD), (dict(out=ODD), BAD), (dict(d=64, out=ODD, ld=772), BAD)],
    "haff_relpos_tables": [(dict(B=0), BAD), (dict(H=0), BAD), (dict(S=0), BAD), (dict(d=0), BAD), (dict(S=-14), BAD),
                           (dict(B=0, dtype=3), BAD), (dict(d=0, dtype=1), BAD)],
    "haff_relpos_tables_bf16": [
        (dict(B=0), BAD), (dict(H=0), BAD), (dict(S=0), BAD), (dict(d=0), BAD), (dict(d=136), BAD), (dict(d=68), BAD), (dict(q_st=84), BAD),
        (dict(q_sh=15684), BAD), (dict(q_sb=31364), BAD), (dict(S=297), UNS), (dict(S=300), UNS), (dict(S=1000, d=8), UNS),
        (dict(S=297, d=136), BAD), (dict(S=297, q_st=84), BAD), (dict(S=300, H=0), BAD)],
    "haff_window_attention": [
        (dict(n_windows=0), BAD), (dict(H=0), BAD), (dict(S=0), BAD), (dict(d=0), BAD), (dict(tab_h=None), BAD), (dict(tab_w=None), BAD),
        (dict(q_st=484), BAD), (dict(k_sb=94084), BAD), (dict(v_sh=84), BAD), (dict(o_st=162), BAD), (dict(o_sh=82), BAD),
        (dict(q=ODD), BAD), (dict(k=F + 328), BAD), (dict(v=F + 648), BAD), (dict(o=F + 4), BAD), (dict(tab_h=ODD), BAD), (dict(tab_w=ODD), BAD),
        (dict(S=7), UNS), (dict(d=64), UNS), (dict(S=16, d=128), UNS), (dict(v_sb=94088), UNS), (dict(v_sh=88), UNS), (dict(v_st=488), UNS),
        (dict(k=F + 640, v=F + 320), UNS), (WIDE, UNS),
        (dict(PADDED, grid_w=56), BAD), (dict(PADDED, n_windows=24), BAD), (dict(PADDED, pad_token=-1), BAD),
        (dict(PADDED, q_st=488), BAD), (dict(PADDED, pad_token=3), BAD), (dict(PADDED, pad_token=4473925), BAD),
        (dict(PADDED, **FAR_V, pad_token=2300000), UNS),
        # a -1 rule and a -2 rule at once: the operand checks come first, then the geometry, then the padded grid's own rules
        (dict(S=7, tab_h=None), BAD), (dict(d=64, q=ODD), BAD), (dict(S=7, q_st=484), BAD), (dict(WIDE, o=F + 4), BAD),
        (dict(PADDED, grid_w=56, S=7), UNS), (dict(PADDED, pad_token=-1, k=F + 640, v=F + 320), UNS), (dict(PADDED, **WIDE, n_windows=24), UNS),
        (dict(PADDED, **FAR_V, pad_token=2300000, grid_w=56), BAD)],
    "haff_attention_bwd": [
        (dict(B=0), BAD), (dict(H=0), BAD), (dict(Nq=0), BAD), (dict(Nk=0), BAD)] + [(dict({x: None}), BAD) for x in BWD_PTRS] + [
        (dict(lse=None), BAD), (dict(workspace=None), BAD), (dict(causal=1, q_pos0=-1), BAD), (dict(ld=260), BAD), (dict(ld=128), BAD)] + [
        (dict({x: ODD}), BAD) for x in BWD_PTRS] + [
        (dict(workspace_elems=BWD_NEED - 1), BAD), (dict(workspace_elems=0), BAD), (dict(workspace=ODD), BAD), (dict(Nq=65), BAD),
        (dict(d=64), UNS), (dict(d=0), UNS), (dict(d=136), UNS),
        # a -1 rule and a -2 rule at once: nulls and the causal rule come before the head dimension, the layout rules after it
        (dict(d=64, q=None), BAD), (dict(d=64, causal=1, q_pos0=-1), BAD), (dict(d=64, ld=260), UNS), (dict(d=64, q=ODD), UNS),
        (dict(d=64, workspace_elems=0), UNS)],
}
for _stem in ("haff_attention_lse", "haff_global_attention", "haff_decode_attention_rope_rows", "haff_window_attention", "haff_attention_bwd"):
    for _dt in ENTRY[_stem][2]:
        CASES[f"{_stem}_{_dt}"] = CASES[_stem]
    del CASES[_stem]


def _entry(name):
    """argument order and base arguments of the exported symbol `name`"""
    for stem, (order, base, dtypes) in ENTRY.items():
        if name in {f"{stem}_{dt}" if dt else stem for dt in dtypes}:
            return order, base
    raise KeyError(name)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(haff.LIB_PATH):
        haff.build_library()
    return haff.load_library()


@pytest.mark.parametrize("name", sorted(CASES))
def test_refusals_and_their_codes(lib, name):
    order, base = _entry(name)
    assert all(want in (BAD, UNS) for _, want in CASES[name])      # nothing here may get as far as a launch
    wrong = []
    for over, want in CASES[name]:
        assert set(over) <= set(base), (name, over)
        args = dict(base, **over)
        got = int(getattr(lib, name)(*[args[k] for k in order]))
        if got != want:
            wrong.append((over, got, want))
    assert not wrong, wrong


def test_both_codes_and_a_doubly_wrong_input_are_recorded_where_the_entry_point_has_them():
    """Every entry point with a -2 rule has a -2 case and a case that breaks a -1 and a -2 rule at once (the plain decode entry points,
    the lse pair, the RoPE decode pair and haff_relpos_tables have no -2 rule ahead of their launch)."""
    only_bad = {n for n in CASES if n.startswith(("haff_attention_lse", "haff_decode_attention_rope_rows", "haff_attention_decode_rows_bf16",
                                                  "haff_attention_decode_rows_f16")) or n == "haff_relpos_tables"}
    for name, cases in CASES.items():
        codes = {want for _, want in cases}
        assert codes == ({BAD} if name in only_bad else {BAD, UNS}), name


def test_every_attention_entry_point_is_covered():
    exported = {n for n in haff.EXPORTED_SYMBOLS if "attention" in n or "relpos" in n}
    assert set(CASES) == exported, set(CASES) ^ exported
