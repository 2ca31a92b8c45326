"""The 16-bit GEMM entry points' host-side contract (no GPU): which inputs each one refuses, and with WHICH code — -1 (bad argument)
or -2 (a geometry the kernels do not serve). The order of the checks is part of the contract: an input that breaks a -1 rule and a
-2 rule at once gets the code of the rule checked first. Every case below is refused before anything is launched (the addresses are
fake, 16-byte aligned and never dereferenced); no case would pass validation. The expected codes were recorded from the library as it
stood before the host half of gemm_bf16.hip was reorganised around named argument setup; they are not derived from the code under test.

The general product (haff_gemm_*, _cfg, _ws, _gather, _ln), _rms and _batched have no -2 rule ahead of their launch, so their
"two rules at once" cases pair the entry point's own check with one of the shared dispatcher's."""
import os

import pytest

import haff

F = 0x1000          # 16-byte aligned, never dereferenced
ODD = F + 8         # 8-byte aligned only
BAD, UNS = -1, -2

GEMM = ("A", "lda", "W", "ldw", "C", "ldc", "bias", "resid", "ldr", "row_map", "M", "N", "K", "act", "out_f32", "swiglu")
GEMM_BASE = dict(A=F, lda=64, W=F, ldw=64, C=F, ldc=64, bias=None, resid=None, ldr=0, row_map=None, M=64, N=64, K=64, act=0,
                 out_f32=0, swiglu=0, stream=None)

# entry point -> (argument order, a base argument set that every case below spoils)
ENTRY = {
    "": (GEMM + ("stream",), GEMM_BASE),
    "_cfg": (GEMM + ("tile_cfg", "stream"), dict(GEMM_BASE, tile_cfg=0)),
    "_ws": (GEMM + ("workspace", "workspace_bytes", "stream"), dict(GEMM_BASE, workspace=F, workspace_bytes=1 << 20)),
    "_gather": (("A", "lda", "a_map", "a_rows") + GEMM[2:] + ("stream",), dict(GEMM_BASE, a_map=F, a_rows=64)),
    "_ln": (GEMM[:10] + ("ln_stats", "ln_colsum") + GEMM[10:] + ("stream",), dict(GEMM_BASE, ln_stats=F, ln_colsum=F)),
    "_rms": (GEMM[:9] + GEMM[10:] + ("ssq_in", "ssq_n", "eps", "ssq_out", "n_parts_out", "stream"),
             dict(GEMM_BASE, M=8, K=128, lda=128, ldw=128, ssq_in=None, ssq_n=0, eps=1e-5, ssq_out=None, n_parts_out=None)),
    "_qkv_rope": (("A", "lda", "W", "ldw", "q_out", "ldq", "kcache", "vcache", "cos_sin", "B", "T", "Tmax", "pos0", "H", "d", "K", "stream"),
                  dict(A=F, lda=256, W=F, ldw=256, q_out=F, ldq=256, kcache=F, vcache=F, cos_sin=F, B=1, T=16, Tmax=32, pos0=0, H=2,
                       d=128, K=256, stream=None)),
    "_rowstats": (("A", "lda", "a_map", "a_rows", "W", "ldw", "C", "ldc", "bias", "resid", "ldr", "M", "N", "K", "stat_out", "stream"),
                  dict(A=F, lda=64, a_map=None, a_rows=0, W=F, ldw=64, C=F, ldc=256, bias=None, resid=F, ldr=256, M=256, N=256, K=64,
                       stat_out=F, stream=None)),
    "_rowstats32": (("A", "lda", "a_map", "a_rows", "W", "ldw", "X32", "ldx", "C", "ldc", "bias", "M", "N", "K", "stat_out", "stream"),
                    dict(A=F, lda=64, a_map=None, a_rows=0, W=F, ldw=64, X32=F, ldx=256, C=F, ldc=256, bias=F, M=256, N=256, K=64,
                         stat_out=F, stream=None)),
    "_heads": (("A", "lda", "W", "ldw", "C", "bias", "row_map", "ln_stats", "ln_colsum", "M", "N", "K", "d", "heads", "part_stride",
                "head_stride", "stream"),
               dict(A=F, lda=64, W=F, ldw=64, C=F, bias=None, row_map=F, ln_stats=None, ln_colsum=None, M=256, N=768, K=64, d=64,
                    heads=4, part_stride=65536, head_stride=16384, stream=None)),
    "_batched": (("A", "lda", "sAo", "sAi", "W", "ldw", "sWo", "sWi", "C", "ldc", "sCo", "sCi", "nb_outer", "nb_inner", "M", "N", "K",
                  "out_f32", "stream"),
                 dict(A=F, lda=64, sAo=0, sAi=0, W=F, ldw=64, sWo=0, sWi=0, C=F, ldc=64, sCo=0, sCi=0, nb_outer=1, nb_inner=1, M=64,
                      N=64, K=64, out_f32=0, stream=None)),
}

# what every entry point refuses with -1: a zero dimension, rows that are no whole 16-byte chunks, misaligned operands
OPERANDS = [(dict(M=0), BAD), (dict(N=0), BAD), (dict(K=0), BAD), (dict(lda=60), BAD), (dict(ldw=60), BAD), (dict(A=ODD), BAD),
            (dict(W=ODD), BAD), (dict(A=ODD, W=ODD, lda=60), BAD)]
# ... and what the entry points with the general epilogue add: K % 8 (the others also have a -2 rule on K), the SwiGLU contract
GENERAL = OPERANDS + [(dict(K=60), BAD), (dict(K=4), BAD), (dict(swiglu=1, N=48), BAD), (dict(swiglu=1, resid=F), BAD),
                      (dict(swiglu=1, ldc=62), BAD), (dict(swiglu=1, N=48, resid=F, K=60), BAD)]
G4 = 1 << 20        # rows that put an operand with a 2048-element leading dimension at exactly 4 GiB
SHAPE256 = [(dict(M=128), UNS), (dict(N=128), UNS), (dict(K=72), UNS), (dict(M=384, N=384, K=96), UNS)]

CASES = {
    "": GENERAL,
    "_cfg": GENERAL + [(dict(tile_cfg=t, K=60), BAD) for t in (1, 2, 3)] + [(dict(tile_cfg=t, M=0, A=ODD), BAD) for t in (1, 2, 3)],
    "_ws": GENERAL + [(dict(workspace=ODD), BAD), (dict(workspace=ODD, workspace_bytes=0), BAD),
                      (dict(workspace=ODD, M=0), BAD), (dict(workspace=ODD, K=60, swiglu=1, N=48), BAD),   # two rules at once
                      (dict(workspace=None, workspace_bytes=0, K=60), BAD)],
    "_gather": GENERAL + [(dict(a_map=None), BAD), (dict(a_rows=0), BAD), (dict(a_rows=-4), BAD), (dict(a_map=None, a_rows=0), BAD),
                          (dict(a_map=None, M=0), BAD), (dict(a_rows=0, lda=60), BAD)],                         # two rules at once
    "_ln": GENERAL + [(dict(ln_stats=None), BAD), (dict(ln_stats=None, ln_colsum=None), BAD),
                      (dict(ln_stats=None, K=60), BAD), (dict(ln_stats=None, swiglu=1, N=48), BAD)],            # two rules at once
    "_rms": OPERANDS + [(dict(M=17), BAD), (dict(M=64), BAD), (dict(K=64), BAD), (dict(K=192), BAD), (dict(K=60), BAD),
                        (dict(ssq_in=F, ssq_n=4, M=9), BAD), (dict(ssq_in=F, ssq_n=513), BAD), (dict(ssq_in=ODD, ssq_n=4), BAD),
                        (dict(ssq_in=F, ssq_n=0), BAD), (dict(ssq_in=F, ssq_n=-1), BAD), (dict(ssq_out=F, out_f32=1), BAD),
                        (dict(ssq_out=F, swiglu=1), BAD), (dict(swiglu=1, N=48), BAD), (dict(swiglu=1, resid=F), BAD),
                        (dict(M=17, K=64, ssq_out=F, out_f32=1), BAD)],                                         # two rules at once
    "_qkv_rope": [(dict(B=0), BAD), (dict(T=0), BAD), (dict(H=0), BAD), (dict(K=0), BAD), (dict(q_out=None), BAD), (dict(kcache=None), BAD),
                  (dict(vcache=None), BAD), (dict(cos_sin=None), BAD), (dict(pos0=-1), BAD), (dict(pos0=17), BAD), (dict(T=33), BAD),
                  (dict(lda=252), BAD), (dict(ldw=252), BAD), (dict(ldq=252), BAD), (dict(A=ODD), BAD), (dict(W=ODD), BAD),
                  (dict(q_out=ODD), BAD), (dict(kcache=ODD), BAD), (dict(vcache=ODD), BAD), (dict(cos_sin=ODD), BAD),
                  (dict(d=64, H=4), UNS), (dict(d=256, H=1), UNS), (dict(H=1), UNS), (dict(H=3), UNS), (dict(K=96), UNS),
                  (dict(B=4096, T=1024, Tmax=1024), UNS),                          # M = 2^22
                  (dict(B=2048, T=1024, Tmax=1024, lda=1024), UNS),                # A: 2^21 rows x 2 KiB = 4 GiB
                  (dict(H=32, ldw=174768), UNS),                                   # Wp: 12288 rows x 349536 B >= 4 GiB
                  # a -1 rule and a -2 rule at once: -1 is checked first
                  (dict(K=252), BAD), (dict(d=64, H=4, kcache=None), BAD), (dict(H=1, pos0=17), BAD), (dict(d=64, K=252), BAD),
                  (dict(B=4096, T=1024, Tmax=1024, cos_sin=ODD), BAD), (dict(B=2048, T=1024, Tmax=1024, lda=1024, ldq=252), BAD)],
    "_rowstats": OPERANDS + SHAPE256 + [
                  (dict(resid=None), BAD), (dict(stat_out=None), BAD), (dict(ldc=252), BAD), (dict(ldr=252), BAD), (dict(C=ODD), BAD),
                  (dict(resid=ODD), BAD), (dict(stat_out=F + 4), BAD),
                  (dict(a_map=F, a_rows=0), UNS), (dict(M=G4, lda=2048), UNS), (dict(a_map=F, a_rows=G4, lda=2048), UNS),
                  (dict(N=G4, ldw=2048), UNS),
                  # a -1 rule and a -2 rule at once: -1 is checked first
                  (dict(K=60), BAD), (dict(M=128, resid=None), BAD), (dict(N=128, ldw=60), BAD), (dict(K=72, stat_out=F + 4), BAD),
                  (dict(a_map=F, a_rows=0, C=ODD), BAD), (dict(M=G4, lda=2048, ldr=252), BAD)],
    "_rowstats32": OPERANDS + SHAPE256 + [
                  (dict(bias=None), BAD), (dict(X32=None), BAD), (dict(C=None), BAD), (dict(stat_out=None), BAD), (dict(ldx=254), BAD),
                  (dict(ldc=252), BAD), (dict(C=ODD), BAD), (dict(X32=ODD), BAD), (dict(bias=ODD), BAD), (dict(stat_out=F + 4), BAD),
                  (dict(a_map=F, a_rows=0), UNS), (dict(M=G4, lda=2048), UNS), (dict(a_map=F, a_rows=G4, lda=2048), UNS),
                  (dict(N=G4, ldw=2048), UNS),
                  # a -1 rule and a -2 rule at once: -1 is checked first
                  (dict(K=60), BAD), (dict(M=128, bias=None), BAD), (dict(N=128, ldx=254), BAD), (dict(K=72, X32=ODD), BAD),
                  (dict(M=G4, lda=2048, bias=ODD), BAD)],
    "_heads": OPERANDS + SHAPE256 + [
                  (dict(row_map=None), BAD), (dict(C=None), BAD), (dict(d=0), BAD), (dict(heads=0), BAD), (dict(part_stride=65532), BAD),
                  (dict(head_stride=16380), BAD), (dict(C=ODD), BAD),
                  (dict(d=68), UNS), (dict(d=4104, heads=1), UNS), (dict(N=1024), UNS), (dict(N=512, heads=3), UNS),
                  (dict(N=65536, heads=1024), UNS),                                # heads * d = 65536
                  (dict(M=G4, lda=2048), UNS), (dict(N=G4 * 3, heads=1024 * 16, ldw=2048), UNS),
                  # a -1 rule and a -2 rule at once: -1 is checked first
                  (dict(K=60), BAD), (dict(d=68, row_map=None), BAD), (dict(N=1024, part_stride=65532), BAD),
                  (dict(N=65536, heads=1024, C=ODD), BAD), (dict(M=G4, lda=2048, head_stride=16380), BAD)],
    "_batched": OPERANDS + [(dict(K=60), BAD), (dict(nb_outer=0), BAD), (dict(nb_inner=0), BAD), (dict(nb_outer=-1), BAD),
                            (dict(sAo=4), BAD), (dict(sAi=4), BAD), (dict(sWo=4), BAD), (dict(sWi=4), BAD),
                            (dict(nb_outer=0, sAo=4), BAD), (dict(sWi=4, W=ODD, out_f32=1), BAD)],              # two rules at once
}
DTYPES = {k: (("bf16",) if k == "_rowstats32" else ("bf16", "f16")) for k in ENTRY}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(haff.LIB_PATH):
        haff.build_library()
    return haff.load_library()


def _call(lib, name, order, args):
    return int(getattr(lib, name)(*[args[k] for k in order]))


@pytest.mark.parametrize("entry", list(ENTRY))
def test_refusals_and_their_codes(lib, entry):
    order, base = ENTRY[entry]
    assert all(want in (BAD, UNS) for _, want in CASES[entry])      # nothing here may get as far as a launch
    wrong = []
    for dt in DTYPES[entry]:
        name = f"haff_gemm_{dt}{entry}"
        for over, want in CASES[entry]:
            assert set(over) <= set(base), (name, over)
            got = _call(lib, name, order, dict(base, **over))
            if got != want:
                wrong.append((name, over, got, want))
    assert not wrong, wrong


def test_every_sixteen_bit_gemm_entry_point_is_covered():
    names = {f"haff_gemm_{dt}{e}" for e in ENTRY for dt in DTYPES[e]}
    exported = {n for n in haff.EXPORTED_SYMBOLS if n.startswith(("haff_gemm_bf16", "haff_gemm_f16"))}
    assert names == exported, names ^ exported


def test_refused_calls_leave_the_stream_cap_table_alone(lib):
    """A refused product neither reads nor changes the per-stream workgroup cap of the stream it was given."""
    stream = 0x7770
    cap = lambda c: int(lib.haff_gemm_stream_cap(stream, c))   # noqa: E731
    assert cap(0) == 256 and cap(64) == 256
    try:
        for entry, (order, base) in ENTRY.items():
            for dt in DTYPES[entry]:
                over, want = CASES[entry][0]
                assert _call(lib, f"haff_gemm_{dt}{entry}", order, dict(base, stream=stream, **over)) == want
        assert cap(0) == 64
    finally:
        assert cap(256) == 64
    assert cap(0) == 256 and int(lib.haff_gemm_stream_cap(None, 0)) == 256
