"""The host-side contract of the pointwise, norm and training family (no GPU): which inputs each of the 52 entry points of train.hip,
elementwise.hip, norm.hip, sam_decoder.hip, frame_ingest.hip and kv_broadcast.hip refuses, and with WHICH code: -1 (bad argument) or -2
(a shape the kernels do not serve). The order of the checks is part of the contract: an input that breaks a -1 rule and a -2 rule at once
gets the code of the rule checked first. Every call below is refused before anything is launched; the device addresses are fake, 16-byte
aligned unless a case says otherwise, and never dereferenced; the arrays an entry point reads or writes on the HOST (mean3 / std3, the
thresholds, *n_parts) are real. The expected codes and the values of haff_colsum_parts were recorded from the library as it stood before
the six files' host halves were reorganised around one storage-type dispatch, one grid rule and one stream cast (built from the parent
commit and loaded through HAFF_LIB_PATH); they are not derived from the code under test."""
import ctypes
import os

import numpy as np
import pytest

import haff

F = 0x10000         # 16-byte aligned, never dereferenced
BAD, UNS = -1, -2
MEAN3 = np.array([123.675, 116.28, 103.53], dtype=np.float32)
STD3 = np.array([58.395, 57.12, 57.375], dtype=np.float32)
TH = np.array([0.0, 0.5], dtype=np.float32)
N_PARTS = ctypes.c_int(-7)     # haff_sumsq_partials writes *n_parts before it looks at the dtype
HOST = dict(mean3=MEAN3.ctypes.data, std3=STD3.ctypes.data, thresholds_host=TH.ctypes.data, n_parts=ctypes.addressof(N_PARTS))

BAD_DTYPES = (2, 4, -1)        # 2 is the norms' own mixed code; no other entry point has it


def entry(order, **base):
    order = order.split()
    base = dict({k: (None if k == "stream" else HOST.get(k, F)) for k in order}, **base)
    assert set(base) == set(order), set(base) ^ set(order)
    return order, base


def each(key, *values, want=BAD, **also):
    return [(dict({key: v}, **also), want) for v in values]


def nulls(*keys):
    return [({k: None}, BAD) for k in keys]


ADAMW = dict(n=64, lr=1e-3, beta1=0.9, beta2=0.95, eps=1e-8, wd=0.0, step=1, gscale=1.0, g_dtype=0, lp_dtype=0)
ADAMW_CASES = (each("n", 0, -1) + each("step", 0, -1) + each("lp_dtype", 1, 2, 4, -2) + each("g_dtype", *BAD_DTYPES)
               + each("g_dtype", *BAD_DTYPES, lp_dtype=-1) + each("g_dtype", *BAD_DTYPES, lp_dtype=3))
MASK_LOSS = dict(n_samples=2, n=1000, wgt=1.0)
ROPE_CACHE = dict(ld=384, B=2, Tq=4, Hq=2, Hkv=1, d=32, Tmax=16, dtype=0)
ROPE_CACHE_CASES = each("B", 0) + each("Tq", 0) + each("d", 8, 24, 33) + each("ld", 4, 385) + each("dtype", *BAD_DTYPES)
RESIZE = dict(N=2, Hs=64, Ws=64, Hc=48, Wc=40, Ho=100, Wo=90)
RESIZE_CASES = each("N", 0) + each("Hc", 0, 65) + each("Wc", 0, 65) + each("Ho", 0) + each("Wo", 0)
NORM = dict(ldx=1024, ldy=1024, rows=4, C=1024, eps=1e-5, dtype=0)
NORM_CASES = (each("rows", 0) + each("C", 0, 1020) + each("ldx", 1028) + each("ldy", 1028) + nulls("w") + each("dtype", -1, 4)
              # C > 8192: no instance is wide enough, -2 for every code the norms serve; the dtype range is judged before that
              + each("dtype", 0, 1, 2, 3, want=UNS, C=8200, ldx=8200, ldy=8200) + each("dtype", -1, 4, C=8200, ldx=8200, ldy=8200)
              + each("C", 8192 + 8, 16384, want=UNS, ldx=16384, ldy=16384) + each("C", 8196, ldx=16384, ldy=16384, dtype=2)
              + [(dict(C=8200, ldx=8200, ldy=8200, w=None), BAD)])
KV = dict(src_row_stride=4096, dst_row_stride=8192, B=3, F=2, P=8, H=64, dtype=0)

ENTRY = {
    # ---- train.hip
    "haff_transpose": entry("in ld_in s_in_o s_in_i out R C Rp Cp nb_outer nb_inner dtype stream", ld_in=40, s_in_o=4000, s_in_i=0, R=33,
                            C=40, Rp=40, Cp=40, nb_outer=2, nb_inner=1, dtype=0),
    "haff_act_fwd": entry("x y n act dtype stream", n=100, act=1, dtype=0),
    "haff_act_bwd": entry("x dy dx n act dtype stream", n=100, act=1, dtype=0),
    "haff_swiglu_fwd": entry("gu y M F dtype stream", M=3, F=32, dtype=0),
    "haff_swiglu_bwd": entry("gu dy dgu M F dtype stream", M=3, F=32, dtype=0),
    "haff_axpby": entry("a b out n alpha beta dtype stream", n=100, alpha=1.0, beta=0.5, dtype=0),
    "haff_scale_dev": entry("a out rows cols alpha alpha_stride dtype stream", rows=4, cols=25, alpha_stride=1, dtype=0),
    "haff_mul": entry("a b out n dtype stream", n=100, dtype=0),
    "haff_norm_bwd": entry("x dy w dx dyx rows C eps rms dtype stream", rows=4, C=4096, eps=1e-5, rms=1, dtype=0),
    "haff_norm_bwd_add": entry("x dy w add dx dyx rows C eps rms dtype stream", rows=4, C=4096, eps=1e-5, rms=1, dtype=0),
    "haff_colsum": entry("x out R C dtype stream", R=2048, C=64, dtype=0),
    "haff_softmax_fwd": entry("s ld p ldp rows Nq Nk scale causal q_pos0 dtype stream", ld=40, ldp=40, rows=12, Nq=6, Nk=33, scale=0.125,
                              causal=1, q_pos0=0, dtype=0),
    "haff_softmax_bwd": entry("p ldp dp ld ds rows Nk scale dtype stream", ldp=40, ld=40, rows=12, Nk=33, scale=0.125, dtype=0),
    "haff_rope": entry("x ldx y ldy cos_sin rows Tlen H d pos0 adjoint dtype stream", ldx=128, ldy=128, rows=8, Tlen=4, H=2, d=64, pos0=0,
                       adjoint=0, dtype=0),
    "haff_cross_entropy": entry("logits ld labels row_loss dlogits rows V gscale dtype stream", ld=1000, rows=4, V=997, gscale=0.25, dtype=0),
    "haff_mask_loss_stats": entry("x t stats n_samples n wgt stream", **MASK_LOSS),
    "haff_mask_loss_grad": entry("x t stats dx n_samples n wgt c_bce c_dice stream", c_bce=2.0, c_dice=0.5, **MASK_LOSS),
    "haff_mask_loss_grad_dev": entry("x t stats dx n_samples n wgt coef stream", **MASK_LOSS),
    "haff_resize_bilinear_bwd": entry("dout din N Hs Ws Hc Wc Ho Wo stream", **RESIZE),
    "haff_scatter_add_rows": entry("ids dx dE rows C dtype stream", rows=10, C=64, dtype=0),
    "haff_reduce_partials": entry("partials out n_out n_parts out_inner part_stride group_stride accumulate stream", n_out=8, n_parts=4,
                                  out_inner=8, part_stride=8, group_stride=0, accumulate=0),
    "haff_sumsq_partials": entry("g partials n dtype n_parts stream", n=1000, dtype=0),
    "haff_mask_loss_stats_partials": entry("x t partials n_samples n wgt n_parts stream", **MASK_LOSS),
    "haff_colsum_partials": entry("x partials R C dtype stream", R=100, C=64, dtype=0),
    "haff_scatter_add_rows_sorted": entry("sorted_ids order dx dE rows C dtype stream", rows=10, C=64, dtype=0),
    "haff_sumsq": entry("g out n dtype stream", n=1000, dtype=0),
    "haff_adamw_step": entry("master m v g param_lp n lr beta1 beta2 eps wd step gscale g_dtype lp_dtype stream", **ADAMW),
    "haff_adamw_step_dev": entry("master m v g param_lp n lr beta1 beta2 eps wd step gscale gscale_dev g_dtype lp_dtype stream", **ADAMW),
    "haff_adamw_step_skip": entry("master m v g param_lp n lr beta1 beta2 eps wd step gscale gscale_dev norm g_dtype lp_dtype stream", **ADAMW),
    "haff_taxonomy_ce": entry("z t probs loss dz rows C stream", rows=5, C=4),
    # ---- elementwise.hip
    "haff_patchify_nchw": entry("x out B Cin Hin Win P gh gw Kp in_dtype out_dtype stream", B=2, Cin=3, Hin=64, Win=48, P=16, gh=4, gw=3,
                                Kp=768, in_dtype=1, out_dtype=0),
    "haff_patchify_u8": entry("frames out B Hf Wf P gh gw Kp mean3 std3 out_dtype stream", B=2, Hf=60, Wf=40, P=16, gh=4, gw=3, Kp=768,
                              out_dtype=0),
    "haff_im2col3x3": entry("x out B H W C dtype stream", B=2, H=8, W=8, C=16, dtype=0),
    "haff_embed_splice": entry("ids img_pos embed img out B L n_img Hd dtype stream", B=2, L=10, n_img=4, Hd=64, dtype=0),
    "haff_rope_cache": entry("qkv ld kcache vcache cos_sin B Tq Hq Hkv d pos0 Tmax dtype stream", pos0=3, **ROPE_CACHE),
    "haff_rope_cache_rows": entry("qkv ld kcache vcache cos_sin B Tq Hq Hkv d pos0_rows Tmax dtype stream", **ROPE_CACHE),
    "haff_argmax_rows": entry("x ld out rows V stream", ld=1000, rows=3, V=997),
    "haff_decode_book": entry("nxt_raw forced forced_ld use_forced steps finished out_ids out_ld lens t_rows tok pos nk h1 hidden hid_sb "
                              "row_bytes pad eos B stream", forced_ld=8, out_ld=64, hid_sb=8192, row_bytes=128, pad=0, eos=2, B=2),
    "haff_add_bcast": entry("a b out rows C mod dtype stream", rows=10, C=64, mod=5, dtype=0),
    "haff_softmax_rows": entry("x out rows C dtype stream", rows=3, C=4, dtype=0),
    # ---- norm.hip
    "haff_layernorm": entry("x ldx y ldy w b in_map rows C eps dtype stream", in_map=None, **NORM),
    "haff_rmsnorm": entry("x ldx y ldy w rows C eps dtype stream", **NORM),
    "haff_row_stats_finalize": entry("partials stats rows slots C eps stream", rows=10, slots=20, C=1280, eps=1e-6),
    "haff_row_stats": entry("x ldx stats rows C eps rms dtype stream", ldx=1024, rows=4, C=1024, eps=1e-5, rms=0, dtype=0),
    # ---- sam_decoder.hip
    "haff_upscale_mask": entry("up1 ln_w ln_b w2 b2 hyper out n_prompts h w eps dtype stream", n_prompts=2, h=8, w=8, eps=1e-6, dtype=0),
    "haff_resize_bilinear": entry("in out N Hs Ws Hc Wc Ho Wo stream", **RESIZE),
    "haff_threshold_masks": entry("in out total logit_th stream", total=1000, logit_th=0.0),
    "haff_gate_threshold_masks": entry("logits planes total plane_stride thresholds_host n_th on_value taxonomy blank_class stream", total=1001,
                                       plane_stride=1004, n_th=2, on_value=255, blank_class=3),
    # ---- frame_ingest.hip
    "haff_resample_u8": entry("in out B Hin Win Hout Wout axis bounds coeffs ksize stream", B=2, Hin=48, Win=64, Hout=48, Wout=32, axis=0,
                              ksize=5),
    "haff_clip_normalize_u8": entry("in out B Hin Win top left S lut out_dtype stream", B=2, Hin=48, Win=64, top=4, left=8, S=40, out_dtype=0),
    # ---- kv_broadcast.hip
    "haff_kv_prefix_broadcast": entry("k_src v_src src_row_stride k_dst v_dst dst_row_stride frame_of B F P H dtype stream", **KV),
}

DT = each("dtype", *BAD_DTYPES)
CASES = {
    "haff_transpose": each("R", 0) + each("C", 0) + each("Rp", 32) + each("Cp", 39) + each("nb_outer", 0) + each("nb_inner", 0, -1) + DT,
    "haff_act_fwd": each("n", 0, -1) + DT,
    "haff_act_bwd": each("n", 0, -1) + DT,
    # dtype 2 with aligned and with misaligned pointers: neither the vector path nor the scalar one has it
    "haff_swiglu_fwd": each("M", 0) + each("F", 0, 8, 24, 33) + DT + each("dtype", *BAD_DTYPES, gu=F + 2),
    "haff_swiglu_bwd": each("M", 0) + each("F", 0, 8, 24, 33) + DT + each("dtype", *BAD_DTYPES, dy=F + 2),
    "haff_axpby": each("n", 0, -1) + DT,
    "haff_scale_dev": each("rows", 0) + each("cols", 0) + nulls("alpha") + each("alpha_stride", 2, -1, 25) + DT,
    "haff_mul": each("n", 0, -1) + DT,
    "haff_norm_bwd": (each("rows", 0) + each("C", 0, -8) + DT + each("dtype", *BAD_DTYPES, C=5120) + each("dtype", *BAD_DTYPES, C=1000)
                      + each("dtype", *BAD_DTYPES, x=F + 2) + each("dtype", *BAD_DTYPES, rms=0)),
    "haff_norm_bwd_add": nulls("add") + each("rows", 0) + each("C", 0) + DT + each("dtype", *BAD_DTYPES, C=1000),
    "haff_colsum": each("R", 0, -1) + each("C", 0) + DT + each("dtype", *BAD_DTYPES, R=100) + each("dtype", *BAD_DTYPES, C=63),
    "haff_softmax_fwd": each("rows", 0) + each("Nq", 0) + each("Nk", 0) + each("ldp", 32) + each("ld", 32) + DT,
    "haff_softmax_bwd": each("rows", 0) + each("Nk", 0) + each("ldp", 32) + each("ld", 32) + DT,
    "haff_rope": each("rows", 0) + each("Tlen", 0) + each("H", 0) + each("d", 0, -2, 1, 63) + DT,
    "haff_cross_entropy": each("rows", 0) + each("V", 0) + each("ld", 996, 0) + DT,
    "haff_mask_loss_stats": each("n_samples", 0, -1) + each("n", 0, -1),
    "haff_mask_loss_grad": each("n_samples", 0, -1) + each("n", 0, -1),
    "haff_mask_loss_grad_dev": each("n_samples", 0, -1) + each("n", 0, -1) + nulls("coef"),
    "haff_resize_bilinear_bwd": RESIZE_CASES,
    "haff_scatter_add_rows": each("rows", 0) + each("C", 0) + DT,
    "haff_reduce_partials": nulls("partials", "out") + each("n_out", 0) + each("n_parts", 0) + each("out_inner", 0),
    "haff_sumsq_partials": each("n", 0, -1) + nulls("partials", "n_parts") + DT,
    "haff_mask_loss_stats_partials": each("n_samples", 0) + each("n", 0) + nulls("partials", "n_parts"),
    "haff_colsum_partials": each("R", 0) + each("C", 0) + nulls("partials") + DT,
    "haff_scatter_add_rows_sorted": each("rows", 0) + each("C", 0) + nulls("sorted_ids", "order") + DT,
    "haff_sumsq": each("n", 0, -1) + DT,
    "haff_adamw_step": ADAMW_CASES,
    "haff_adamw_step_dev": ADAMW_CASES + nulls("gscale_dev"),
    "haff_adamw_step_skip": ADAMW_CASES + nulls("norm") + [(dict(gscale_dev=None, step=0), BAD)],
    "haff_taxonomy_ce": each("rows", 0) + each("C", 0, 9, 16),
    "haff_patchify_nchw": (each("B", 0) + each("P", 0) + each("gh", 5) + each("gw", 4) + each("Kp", 767)
                           + [(dict(in_dtype=i, out_dtype=o), BAD) for i, o in ((0, 3), (3, 0), (3, 1), (2, 0), (0, 2), (2, 2), (4, 4), (-1, 0), (1, 4))]),
    "haff_patchify_u8": each("B", 0) + each("P", 0) + each("Kp", 767) + nulls("mean3", "std3") + each("out_dtype", *BAD_DTYPES),
    "haff_im2col3x3": each("B", 0) + each("C", 4, 17) + DT,
    "haff_embed_splice": each("B", 0) + each("L", 0) + each("n_img", 0) + each("Hd", 4, 65) + DT,
    "haff_rope_cache": ROPE_CACHE_CASES + each("pos0", -1, 13),
    "haff_rope_cache_rows": ROPE_CACHE_CASES + nulls("pos0_rows") + each("Tq", 17),
    "haff_argmax_rows": each("rows", 0, -1) + each("V", 0, -1),
    "haff_decode_book": (each("B", 0, -1) + nulls("nxt_raw", "use_forced", "steps", "finished", "out_ids", "lens", "t_rows", "tok", "pos", "nk")
                         + each("row_bytes", 120, 8) + each("hid_sb", 8200) + each("h1", F + 8, F + 1) + each("hidden", F + 8, F + 4)),
    "haff_add_bcast": each("rows", 0) + each("C", 4, 65) + each("mod", 0, -1) + DT,
    "haff_softmax_rows": each("rows", 0) + each("C", 0) + DT,
    "haff_layernorm": NORM_CASES + nulls("b"),
    "haff_rmsnorm": NORM_CASES,
    "haff_row_stats_finalize": each("rows", 0) + each("slots", 0) + each("C", 0) + nulls("partials", "stats"),
    "haff_row_stats": (each("rows", 0) + each("C", 0, 1020) + each("ldx", 1028) + nulls("stats") + DT
                       # C > 8192: -2 from the codes that have kernels, in either form; code 2 has none here and is refused first with -1
                       + each("dtype", 0, 1, 3, want=UNS, C=8200, ldx=8200) + each("dtype", 0, 1, 3, want=UNS, C=8200, ldx=8200, rms=1)
                       + each("dtype", 2, 4, -1, C=8200, ldx=8200) + each("dtype", 2, C=8200, ldx=8200, rms=1)
                       + [(dict(C=8200, ldx=8200, stats=None), BAD), (dict(C=8200, ldx=8204), BAD)]),
    "haff_upscale_mask": each("n_prompts", 0) + each("h", 0) + each("w", 0) + DT,
    "haff_resize_bilinear": RESIZE_CASES,
    "haff_threshold_masks": each("total", 0, -1),
    "haff_gate_threshold_masks": (each("total", 0) + each("n_th", 0, 9) + each("on_value", -1, 256) + nulls("thresholds_host")
                                  + each("logits", F + 4, F + 8) + each("planes", F + 1, F + 2) + each("plane_stride", 1000, 1002, 1005)),
    "haff_resample_u8": (each("B", 0) + each("Hin", 0) + each("Win", 0) + each("Hout", 0, 47) + each("Wout", 0) + each("ksize", 0)
                         + nulls("bounds", "coeffs") + each("axis", 2, -1) + each("axis", 1) + each("axis", 1, Wout=64, Hout=24, Win=63)),
    "haff_clip_normalize_u8": (each("B", 0) + each("S", 0, 45) + each("top", -1, 9) + each("left", -1, 25) + nulls("lut")
                               + each("out_dtype", *BAD_DTYPES)),
    "haff_kv_prefix_broadcast": (nulls("k_src", "v_src", "k_dst", "v_dst", "frame_of") + each("B", 0) + each("F", 0) + each("P", 0) + each("H", 0)
                                 + DT + each("H", 4, 60) + each("H", 4, dtype=3) + each("H", 2, dtype=1) + each("src_row_stride", 511, 0)
                                 + each("dst_row_stride", 511) + each("src_row_stride", 4100) + each("dst_row_stride", 8196)
                                 + each("src_row_stride", 4098, dtype=1) + each("k_src", F + 8) + each("v_src", F + 2) + each("k_dst", F + 4)
                                 + each("v_dst", F + 8) + each("frame_of", F + 2)
                                 # more workgroups than a grid's x holds: -2, after every -1 rule
                                 + [(dict(B=2 ** 31 - 1, P=1024, H=16, src_row_stride=16384, dst_row_stride=16384), UNS),
                                    (dict(B=2 ** 31 - 1, P=1024, H=16, src_row_stride=16384, dst_row_stride=16384, frame_of=F + 2), BAD),
                                    (dict(B=2 ** 31 - 1, P=1024, H=16, src_row_stride=16384, dst_row_stride=16384, dtype=2), BAD)]),
}

# haff_colsum_parts(R): the row blocks of the ordered column sums (pure host arithmetic)
COLSUM_PARTS = {-1: 0, 0: 0, 1: 1, 63: 1, 64: 1, 65: 2, 4096: 64, 4097: 241, 65536: 256, 65537: 256, 1000000: 256}

HAS_UNS = ("haff_layernorm", "haff_rmsnorm", "haff_row_stats", "haff_kv_prefix_broadcast")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(haff.LIB_PATH):
        haff.build_library()
    return haff.load_library()


def test_every_entry_point_of_the_six_files_has_cases():
    assert len(ENTRY) == 51 and set(CASES) == set(ENTRY)       # the 52nd, haff_colsum_parts, returns a count, not a code


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
        assert {want for _, want in cases} == ({BAD, UNS} if name in HAS_UNS else {BAD}), name


def test_sumsq_partials_writes_its_part_count_before_it_judges_the_dtype(lib):
    order, base = ENTRY["haff_sumsq_partials"]
    for n, parts in ((1, 1), (256, 1), (257, 2), (1024 * 256, 1024), (1024 * 256 + 1, 1024)):
        N_PARTS.value = -7
        assert lib.haff_sumsq_partials(*[dict(base, n=n, dtype=2)[k] for k in order]) == BAD
        assert N_PARTS.value == parts, (n, N_PARTS.value)
    N_PARTS.value = -7
    assert lib.haff_sumsq_partials(*[dict(base, n=0, dtype=2)[k] for k in order]) == BAD and N_PARTS.value == -7


@pytest.mark.parametrize("R", sorted(COLSUM_PARTS))
def test_colsum_parts(lib, R):
    assert lib.haff_colsum_parts(R) == COLSUM_PARTS[R]
