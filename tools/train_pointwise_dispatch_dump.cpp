// Host-only dump of what the pointwise, norm and training family WOULD launch: every hipLaunchKernelGGL in csrc/train.hip,
// elementwise.hip, norm.hip, sam_decoder.hip, frame_ingest.hip and kv_broadcast.hip becomes a record in text (kernel, grid, block,
// dynamic LDS bytes, every argument) and every entry-point call an `rc` line (with *n_parts where an entry point writes it), over a
// sweep that reaches both sides of every host branch: every dtype code, aligned and misaligned operands of the vector paths, the
// norm_bwd / colsum_vec / launch_norm predicates' edges, every nch rung, the six patchify pairs and grids on both sides of every cap.
// The device addresses are fake, one 2^40 range per role, never dereferenced, and printed as role+offset. Nothing is launched and no
// GPU is needed. The files' anonymous namespaces clash in one unit, so build it once per file (-DDUMP_TU=1..6) and concatenate the
// outputs; two builds against two versions of the sources must print identical output when the host dispatch is unchanged:
//   for t in 1 2 3 4 5 6; do hipcc -std=c++17 -x hip --cuda-host-only -Wl,--unresolved-symbols=ignore-all -DDUMP_TU=$t \
//       -I<csrc dir to dump> -Iinclude tools/train_pointwise_dispatch_dump.cpp -o dump$t; done
//   (for t in 1 2 3 4 5 6; do ./dump$t; done) | sha256sum
// A kernel is named by its INSTANCE, not by the text at its launch: the launch macro hands the kernel to dump_launch as a template
// argument and the record carries its mangled name (..._GLOBAL__N_116transpose_kernelItEEv...: the name, its template arguments, its
// parameter types), so `<T>` inside a dispatch macro and `<bf16_t>` written out give the same record. Taking a kernel's address makes the host-only unit refer to a device binary that is never built: hence the
// linker flag.
#include <hip/hip_runtime.h>
#include <cstdarg>
#include <cstdio>
#include <type_traits>
#include <typeinfo>
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) dump_launch<kernel>(grid, block, (size_t)(shmem), __VA_ARGS__)
#define hipGetLastError() hipSuccess
template <auto K, typename... A> static void dump_launch(dim3 g, dim3 b, size_t lds, const A&... a);

#ifndef DUMP_TU
#error "build with -DDUMP_TU=1 (train.hip), 2 (elementwise.hip), 3 (norm.hip), 4 (sam_decoder.hip), 5 (frame_ingest.hip) or 6 (kv_broadcast.hip)"
#elif DUMP_TU == 1
#include "train.hip"
#elif DUMP_TU == 2
#include "elementwise.hip"
#elif DUMP_TU == 3
#include "norm.hip"
#elif DUMP_TU == 4
#include "sam_decoder.hip"
#elif DUMP_TU == 5
#include "frame_ingest.hip"
#else
#include "kv_broadcast.hip"
#endif

static long n_records = 0;

// fake device addresses: role r (1..31) owns [r << 40, (r + 1) << 40); A(r) is its base, A(r, off) a byte offset into it
static char* A(unsigned long role, long off = 0) { return reinterpret_cast<char*>(role << 40) + off; }

static void dump_ptr(const void* p) {
  const unsigned long a = reinterpret_cast<unsigned long>(p);
  if (!a) printf(" null");
  else if ((a >> 40) < 32) printf(" r%lu+%lu", a >> 40, a & ((1UL << 40) - 1));
  else printf(" HOST");   // a host address in a kernel argument would be a bug: make it show
}
#if DUMP_TU == 2
static void dump_arg(const DecodeBookArgs& p) {
  for (const void* q : {(const void*)p.nxt_raw, (const void*)p.forced}) dump_ptr(q);
  printf(" %ld", p.forced_ld);
  for (const void* q : {(const void*)p.use_forced, (const void*)p.steps, (const void*)p.finished, (const void*)p.out_ids}) dump_ptr(q);
  printf(" %ld", p.out_ld);
  for (const void* q : {(const void*)p.lens, (const void*)p.t_rows, (const void*)p.tok, (const void*)p.pos, (const void*)p.nk,
                        (const void*)p.h1, (const void*)p.hidden})
    dump_ptr(q);
  printf(" %ld %ld %ld %ld", p.hid_sb, p.row_bytes, p.pad, p.eos);
}
#elif DUMP_TU == 4
static void dump_arg(const GateArgs& p) {
  dump_ptr(p.in); dump_ptr(p.out);
  printf(" %ld %ld", p.total, p.plane_stride);
  dump_ptr(p.taxonomy);
  printf(" %d %d %d", p.blank_class, p.n_th, p.on_value);
  for (float v : p.th) printf(" %a", (double)v);
}
#endif
template <typename T> static void dump_arg(const T& v) {
  if constexpr (std::is_null_pointer<T>::value) printf(" null");
  else if constexpr (std::is_pointer<T>::value) dump_ptr(v);
  else if constexpr (std::is_floating_point<T>::value) printf(" %a", (double)v);
  else printf(" %lld", (long long)v);
}

template <auto K> struct KernelTag {};
template <auto K, typename... A> static void dump_launch(dim3 g, dim3 b, size_t lds, const A&... a) {
  ++n_records;
  // the tag type's mangled name holds the kernel's with its template arguments (__PRETTY_FUNCTION__ leaves those out)
  printf("launch %s grid %u %u %u block %u %u %u lds %zu args", typeid(KernelTag<K>).name(), g.x, g.y, g.z, b.x, b.y, b.z, lds);
  (dump_arg(a), ...);
  printf("\n");
}

// one `rc` line per entry-point call, after the launch record the call made (if any)
static void rc(int code, const char* fmt, ...) {
  ++n_records;
  va_list ap;
  va_start(ap, fmt);
  printf("rc ");
  vprintf(fmt, ap);
  va_end(ap);
  printf(" -> %d\n", code);
}

static const int kDtypes[] = {0, 1, 3, 2, 4};                 // bf16, f32, f16; the norms' mixed code; no code at all
static const long kMis[] = {0, 2, 8};                         // a 16-byte boundary; a 2-byte one; an 8-byte one

#if DUMP_TU == 1
static void sweep() {
  void* const s = nullptr;
  const long cap = 16384L * 256;
  for (int dt : kDtypes) {
    const int shapes[][6] = {{33, 40, 40, 40, 2, 1}, {1, 1, 1, 1, 1, 1}, {100, 70, 104, 72, 2, 3}, {32, 64, 32, 64, 1, 1}};
    for (const auto& q : shapes)
      rc(haff_transpose(A(1), 80, 8000, 16, A(2), q[0], q[1], q[2], q[3], q[4], q[5], dt, s), "transpose %d %d %d %d %d %d dt %d", q[0], q[1],
         q[2], q[3], q[4], q[5], dt);
    for (long n : {1L, 256L, 257L, cap - 256, cap, cap + 1, 10 * cap}) {
      rc(haff_act_fwd(A(1), A(2), n, 1, dt, s), "act_fwd n %ld dt %d", n, dt);
      rc(haff_act_bwd(A(1), A(2), A(3), n, 4, dt, s), "act_bwd n %ld dt %d", n, dt);
      rc(haff_axpby(A(1), n & 1 ? nullptr : A(2), A(3), n, 0.5f, 2.f, dt, s), "axpby n %ld dt %d", n, dt);
      rc(haff_mul(A(1), A(2), A(3), n, dt, s), "mul n %ld dt %d", n, dt);
      rc(haff_scale_dev(A(1), A(2), 1, n, reinterpret_cast<float*>(A(3)), 0, dt, s), "scale_dev 1 x %ld dt %d", n, dt);
      rc(haff_scale_dev(A(1), A(2), n, 3, reinterpret_cast<float*>(A(3)), 1, dt, s), "scale_dev %ld x 3 dt %d", n, dt);
      rc(haff_scatter_add_rows(reinterpret_cast<long*>(A(1)), A(2), reinterpret_cast<float*>(A(3)), n, 1, dt, s), "scatter_add_rows %ld x 1 dt %d", n, dt);
      rc(haff_scatter_add_rows(reinterpret_cast<long*>(A(1)), A(2), reinterpret_cast<float*>(A(3)), 7, (int)(n > 1 << 20 ? 1 << 20 : n), dt, s),
         "scatter_add_rows 7 x min(%ld, 2^20) dt %d", n, dt);
      rc(haff_scatter_add_rows_sorted(reinterpret_cast<long*>(A(1)), reinterpret_cast<long*>(A(2)), A(3), reinterpret_cast<float*>(A(4)), n, 64, dt, s),
         "scatter_add_rows_sorted %ld dt %d", n, dt);
    }
    // swiglu: the vector path's grid meets the cap at M * F = 2^25, the scalar one's at 2^22
    for (long M : {1L, 3L, 16384L, 16385L, 131072L, 131073L})
      for (int F : {16, 256})
        for (int which = 0; which < 4; ++which)
          for (long mis : kMis) {
            if ((which == 0) != (mis == 0)) continue;         // which: no operand off its boundary, or the first, second, third
            const long o1 = which == 1 ? mis : 0, o2 = which == 2 ? mis : 0, o3 = which == 3 ? mis : 0;
            if (which < 3) rc(haff_swiglu_fwd(A(1, o1), A(2, o2), M, F, dt, s), "swiglu_fwd %ld x %d dt %d off %ld %ld", M, F, dt, o1, o2);
            rc(haff_swiglu_bwd(A(1, o1), A(2, o2), A(3, o3), M, F, dt, s), "swiglu_bwd %ld x %d dt %d off %ld %ld %ld", M, F, dt, o1, o2, o3);
          }
    // norm_bwd: C in {4096, 5120, other} x rms x add; every operand off its boundary in turn; w, dyx, add null
    for (int C : {4096, 5120, 1024, 4104, 8})
      for (int rms = 0; rms < 2; ++rms)
        for (int rows : {1, 4, 5})
          for (int which = 0; which < 9; ++which) {           // 0: all aligned; 1..6: one of x dy w add dx dyx off; 7: w null; 8: dyx null
            long o[7] = {0, 0, 0, 0, 0, 0, 0};
            if (which >= 1 && which <= 6) o[which] = which & 1 ? 8 : 4;
            const float* w = which == 7 ? nullptr : reinterpret_cast<const float*>(A(3, o[3]));
            float* dyx = which == 8 ? nullptr : reinterpret_cast<float*>(A(6, o[6]));
            if (which != 4)
              rc(haff_norm_bwd(A(1, o[1]), A(2, o[2]), w, A(5, o[5]), dyx, rows, C, 1e-5f, rms, dt, s), "norm_bwd rows %d C %d rms %d dt %d which %d",
                 rows, C, rms, dt, which);
            rc(haff_norm_bwd_add(A(1, o[1]), A(2, o[2]), w, A(4, o[4]), A(5, o[5]), dyx, rows, C, 1e-5f, rms, dt, s),
               "norm_bwd_add rows %d C %d rms %d dt %d which %d", rows, C, rms, dt, which);
          }
    // colsum: the vector path wants C a power-of-two multiple of 8 up to 2048, R >= 1024 and an aligned x
    for (int C : {1, 8, 16, 24, 63, 64, 1024, 2048, 4096, 2056})
      for (long R : {1L, 1023L, 1024L, 5000L, 100000L, 1L << 22})
        for (long mis : kMis)
          rc(haff_colsum(A(1, mis), reinterpret_cast<float*>(A(2)), R, C, dt, s), "colsum %ld x %d dt %d off %ld", R, C, dt, mis);
    for (long R : {1L, 63L, 64L, 65L, 4096L, 4097L, 100000L})
      for (int C : {1, 64, 65})
        rc(haff_colsum_partials(A(1), reinterpret_cast<float*>(A(2)), R, C, dt, s), "colsum_partials %ld x %d dt %d", R, C, dt);
    for (long rows : {1L, 4L, 5L, 1000L}) {
      rc(haff_softmax_fwd(reinterpret_cast<float*>(A(1)), 40, A(2), 48, rows, 5, 33, 0.125f, 1, 2, dt, s), "softmax_fwd rows %ld dt %d", rows, dt);
      rc(haff_softmax_bwd(A(1), 48, reinterpret_cast<float*>(A(2)), 40, A(3), rows, 33, 0.125f, dt, s), "softmax_bwd rows %ld dt %d", rows, dt);
      rc(haff_cross_entropy(A(1), 1000, reinterpret_cast<long*>(A(2)), reinterpret_cast<float*>(A(3)), A(4), rows, 997, 0.25f, dt, s),
         "cross_entropy rows %ld dt %d", rows, dt);
    }
    for (long rows : {1L, 8L, 65532L, 65536L, 65537L})        // rows * H * d / 2 = 64 rows: the cap at 65536 rows
      for (int adj = 0; adj < 2; ++adj)
        rc(haff_rope(A(1), 128, A(2), 136, reinterpret_cast<float*>(A(3)), rows, 4, 2, 64, 3, adj, dt, s), "rope rows %ld adjoint %d dt %d", rows, adj, dt);
    for (long n : {1L, 256L, 257L, 261888L, 262144L, 262145L, 1L << 30}) {   // the cap of 1024 blocks
      int parts = -7;
      rc(haff_sumsq_partials(A(1), reinterpret_cast<float*>(A(2)), n, dt, &parts, s), "sumsq_partials n %ld dt %d", n, dt);
      printf("n_parts %d\n", parts);
      rc(haff_sumsq(A(1), reinterpret_cast<float*>(A(2)), n, dt, s), "sumsq n %ld dt %d", n, dt);
    }
    for (int lp : {-1, 0, 3, 1})
      for (long n : {1L, 256L, 257L, cap, cap + 1}) {
        float* const F32[] = {reinterpret_cast<float*>(A(1)), reinterpret_cast<float*>(A(2)), reinterpret_cast<float*>(A(3)),
                              reinterpret_cast<float*>(A(6)), reinterpret_cast<float*>(A(7))};
        rc(haff_adamw_step(F32[0], F32[1], F32[2], A(4), A(5), n, 1e-3f, .9f, .95f, 1e-8f, .01f, 3, .5f, dt, lp, s), "adamw n %ld g %d lp %d", n, dt, lp);
        rc(haff_adamw_step_dev(F32[0], F32[1], F32[2], A(4), A(5), n, 1e-3f, .9f, .95f, 1e-8f, .01f, 3, .5f, F32[3], dt, lp, s),
           "adamw_dev n %ld g %d lp %d", n, dt, lp);
        for (int dev = 0; dev < 2; ++dev)
          rc(haff_adamw_step_skip(F32[0], F32[1], F32[2], A(4), A(5), n, 1e-3f, .9f, .95f, 1e-8f, .01f, 3, .5f, dev ? F32[3] : nullptr, F32[4], dt,
                                  lp, s),
             "adamw_skip n %ld g %d lp %d dev %d", n, dt, lp, dev);
      }
  }
  const float* const x = reinterpret_cast<float*>(A(1));
  const float* const t = reinterpret_cast<float*>(A(2));
  for (long n : {1L, 256L, 257L, 65280L, 65536L, 65537L, 1L << 24})   // the cap of 256 blocks
    for (int ns : {1, 3}) {
      rc(haff_mask_loss_stats(x, t, reinterpret_cast<float*>(A(3)), ns, n, .5f, s), "mask_loss_stats %d x %ld", ns, n);
      rc(haff_mask_loss_grad(x, t, reinterpret_cast<float*>(A(3)), reinterpret_cast<float*>(A(4)), ns, n, .5f, 2.f, .25f, s), "mask_loss_grad %d x %ld", ns, n);
      rc(haff_mask_loss_grad_dev(x, t, reinterpret_cast<float*>(A(3)), reinterpret_cast<float*>(A(4)), ns, n, .5f, reinterpret_cast<float*>(A(5)), s),
         "mask_loss_grad_dev %d x %ld", ns, n);
      int parts = -7;
      rc(haff_mask_loss_stats_partials(x, t, reinterpret_cast<float*>(A(3)), ns, n, .5f, &parts, s), "mask_loss_stats_partials %d x %ld", ns, n);
      printf("n_parts %d\n", parts);
    }
  for (int Wc : {1, 2047, 2048, 2049})                        // N * Hc * Wc = 2048 Wc: the cap at Wc = 2048
    rc(haff_resize_bilinear_bwd(x, reinterpret_cast<float*>(A(2)), 1, 2048, 4096, 2048, Wc, 1000, 900, s), "resize_bilinear_bwd Wc %d", Wc);
  for (int n_out : {1, 8, 1000})
    for (int acc = 0; acc < 2; ++acc)
      rc(haff_reduce_partials(x, reinterpret_cast<float*>(A(2)), n_out, 5, 4, 4, 1024, acc, s), "reduce_partials %d acc %d", n_out, acc);
  for (long R : {-1L, 0L, 1L, 63L, 64L, 65L, 4096L, 4097L, 65536L, 65537L, 1000000L}) printf("colsum_parts %ld -> %d\n", R, haff_colsum_parts(R));
  for (int rows : {1, 64, 65, 1000})
    for (int C : {1, 4, 8})
      rc(haff_taxonomy_ce(x, t, reinterpret_cast<float*>(A(3)), reinterpret_cast<float*>(A(4)), reinterpret_cast<float*>(A(5)), rows, C, s),
         "taxonomy_ce %d x %d", rows, C);
}

#elif DUMP_TU == 2
static void sweep() {
  void* const s = nullptr;
  const float mean3[3] = {123.675f, 116.28f, 103.53f}, std3[3] = {58.395f, 57.12f, 57.375f};
  const long cap = 8192L * 256;
  for (int in : kDtypes)
    for (int out : kDtypes)
      for (int gw : {1, 3, 2730, 2731})                       // total = gw * 768: the cap between gw = 2730 and 2731
        rc(haff_patchify_nchw(A(1), A(2), 1, 3, 16, 16 * gw, 16, 1, gw, 768, in, out, s), "patchify_nchw gw %d in %d out %d", gw, in, out);
  for (int dt : kDtypes) {
    for (int gw : {1, 3, 2730, 2731})
      rc(haff_patchify_u8(A(1), A(2), 1, 15, 16 * gw - 3, 16, 1, gw, 776, mean3, std3, dt, s), "patchify_u8 gw %d dt %d", gw, dt);
    for (int W : {1, 8, 14561, 14564})                        // total = 144 W: 8191 blocks, and the cap passed
      rc(haff_im2col3x3(A(1), A(2), 1, 8, W, 16, dt, s), "im2col3x3 W %d dt %d", W, dt);
    for (int L : {1, 10})
      for (int n_img : {1, 4})
        rc(haff_embed_splice(reinterpret_cast<long*>(A(1)), reinterpret_cast<int*>(A(2)), A(3), A(4), A(5), 3, L, n_img, 64, dt, s),
           "embed_splice L %d n_img %d dt %d", L, n_img, dt);
    for (int Tq : {1, 4, 8191, 8192, 8193})                        // total = B Tq (Hq + 2 Hkv) d / 16 = 256 Tq: the cap at Tq = 8192
      for (int pos0 : {0, 5}) {
        rc(haff_rope_cache(A(1), 4096, A(2), A(3), reinterpret_cast<float*>(A(4)), 2, Tq, 32, 16, 32, pos0, 16384, dt, s), "rope_cache Tq %d pos0 %d dt %d",
           Tq, pos0, dt);
        rc(haff_rope_cache_rows(A(1), 4096, A(2), A(3), reinterpret_cast<float*>(A(4)), 2, Tq, 32, 16, 32, reinterpret_cast<int*>(A(5, 4L * pos0)), 16384,
                                dt, s),
           "rope_cache_rows Tq %d rows+%d dt %d", Tq, 4 * pos0, dt);
      }
    for (long rows : {1L, cap - 256, cap - 255, cap, cap + 1})   // total = rows: C / 8 = 1
      rc(haff_add_bcast(A(1), A(2), A(3), rows, 8, 5, dt, s), "add_bcast rows %ld dt %d", rows, dt);
    for (int rows : {1, 64, 65, 1000}) rc(haff_softmax_rows(A(1), reinterpret_cast<float*>(A(2)), rows, 4, dt, s), "softmax_rows %d dt %d", rows, dt);
  }
  for (int rows : {1, 3, 64}) rc(haff_argmax_rows(reinterpret_cast<float*>(A(1)), 32008, reinterpret_cast<long*>(A(2)), rows, 32003, s), "argmax_rows %d", rows);
  for (int B : {1, 5})
    for (int h1 = 0; h1 < 2; ++h1)
      rc(haff_decode_book(reinterpret_cast<long*>(A(1)), reinterpret_cast<long*>(A(2)), 8, reinterpret_cast<int*>(A(3)), reinterpret_cast<int*>(A(4)),
                          reinterpret_cast<unsigned char*>(A(5)), reinterpret_cast<long*>(A(6)), 64, reinterpret_cast<long*>(A(7)),
                          reinterpret_cast<int*>(A(8)), reinterpret_cast<long*>(A(9)), reinterpret_cast<int*>(A(10)), reinterpret_cast<int*>(A(11)),
                          h1 ? A(12) : nullptr, A(13), 8192 + (h1 ? 0 : 8), 128 + (h1 ? 0 : 8), 0, 2, B, s),
         "decode_book B %d h1 %d", B, h1);
}

#elif DUMP_TU == 3
static void sweep() {
  void* const s = nullptr;
  const float* const w = reinterpret_cast<float*>(A(3));
  const float* const b = reinterpret_cast<float*>(A(4));
  // every nch rung (512 columns each: 1 2 3 4 8 10 16 and none) and the one-workgroup-per-row window rows <= 256, 2048 <= C <= 6144
  for (int C : {8, 512, 520, 1024, 1032, 1536, 1544, 2040, 2048, 2056, 4096, 4104, 5120, 5128, 6144, 6152, 8192, 8200})
    for (int rows : {1, 4, 5, 256, 257})
      for (int dt : kDtypes) {
        for (int map = 0; map < 2; ++map)
          rc(haff_layernorm(A(1), C + 8, A(2), C + 16, w, b, map ? reinterpret_cast<int*>(A(5)) : nullptr, rows, C, 1e-6f, dt, s),
             "layernorm rows %d C %d dt %d map %d", rows, C, dt, map);
        rc(haff_rmsnorm(A(1), C + 8, A(2), C + 16, w, rows, C, 1e-5f, dt, s), "rmsnorm rows %d C %d dt %d", rows, C, dt);
        for (int rms = 0; rms < 2; ++rms)
          rc(haff_row_stats(A(1), C + 8, reinterpret_cast<float*>(A(2)), rows, C, 1e-5f, rms, dt, s), "row_stats rows %d C %d rms %d dt %d", rows, C, rms, dt);
      }
  for (int rows : {1, 256, 257, 4096})
    rc(haff_row_stats_finalize(w, reinterpret_cast<float*>(A(2)), rows, 20, 1280, 1e-6f, s), "row_stats_finalize %d", rows);
}

#elif DUMP_TU == 4
static void sweep() {
  void* const s = nullptr;
  const float* const f = reinterpret_cast<float*>(A(2));
  for (int dt : kDtypes)
    for (int h : {1, 8, 64})
      for (int n : {1, 3})
        rc(haff_upscale_mask(A(1), f, f + 64, f + 128, f + 8320, f + 8352, reinterpret_cast<float*>(A(3)), n, h, 64, 1e-6f, dt, s),
           "upscale_mask n %d h %d dt %d", n, h, dt);
  for (int Wo : {1, 1000, 2047, 2048, 2049})                  // N * Ho * Wo = 2048 Wo: the cap of 16384 blocks at Wo = 2048
    rc(haff_resize_bilinear(f, reinterpret_cast<float*>(A(3)), 2, 256, 256, 200, 150, 1024, Wo, s), "resize_bilinear Wo %d", Wo);
  for (long total : {1L, 255L, 256L, 257L, (16384L << 8) - 256, 16384L << 8, (16384L << 8) + 1})
    rc(haff_threshold_masks(f, A(3), total, 0.25f, s), "threshold_masks %ld", total);
  const float th[8] = {-2.f, -1.f, -.5f, 0.f, .25f, .5f, 1.f, 2.f};
  for (long total : {1L, 3L, 4L, 1023L, 1024L, 1025L, 1028L, (8192L << 10) - 1024, 8192L << 10, (8192L << 10) + 4})   // 4 pixels per thread, the cap 8192
    for (int n_th : {1, 8})
      for (int tax = 0; tax < 2; ++tax)
        rc(haff_gate_threshold_masks(f, A(3, 4), total, (total + 3) & ~3L, th, n_th, 255, tax ? reinterpret_cast<float*>(A(4)) : nullptr, 3, s),
           "gate_threshold_masks %ld n_th %d tax %d", total, n_th, tax);
}

#elif DUMP_TU == 5
static void sweep() {
  void* const s = nullptr;
  const int* const bounds = reinterpret_cast<int*>(A(3));
  const int* const coeffs = reinterpret_cast<int*>(A(4));
  for (int Wout : {1, 100, 4095, 4096, 4097}) {               // rows * Wout = 4096 Wout: the cap of 65536 blocks at Wout = 4096
    rc(haff_resample_u8(A(1), A(2), 2, 2048, 5000, 2048, Wout, 0, bounds, coeffs, 7, s), "resample_u8 axis 0 Wout %d", Wout);
    rc(haff_resample_u8(A(1), A(2), 2, 2048, 5000, 2048, Wout, 2, bounds, coeffs, 7, s), "resample_u8 axis 2 Wout %d", Wout);
  }
  for (int Hout : {1, 100, 2730, 2731})                       // B * Hout * 3 Win = 6144 Hout: the cap between 2730 and 2731
    rc(haff_resample_u8(A(1), A(2), 2, 3000, 1024, Hout, 1024, 1, bounds, coeffs, 7, s), "resample_u8 axis 1 Hout %d", Hout);
  for (int dt : kDtypes)
    for (int S : {1, 224, 336, 2364, 2365})                   // B * 3 * S * S = 3 S^2: the cap between S = 2364 and 2365
      rc(haff_clip_normalize_u8(A(1), A(2), 1, 2400, 2400, 7, 9, S, reinterpret_cast<float*>(A(3)), dt, s), "clip_normalize_u8 S %d dt %d", S, dt);
}

#else
static void sweep() {
  void* const s = nullptr;
  for (int dt : kDtypes)
    for (int P : {1, 7, 64, 65, 1000})                        // units = P * H * elem / 16: chunks of 1024 units
      for (int H : {8, 128, 4096})
        for (int B : {1, 3})
          rc(haff_kv_prefix_broadcast(A(1), A(2), 2048L * H, A(3), A(4), 4096L * H, reinterpret_cast<int*>(A(5, 4)), B, 2, P, H, dt, s),
             "kv_prefix_broadcast P %d H %d B %d dt %d", P, H, B, dt);
}
#endif

int main() {
  sweep();
  fprintf(stderr, "%ld records\n", n_records);
  return 0;
}
