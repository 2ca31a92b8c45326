// Host-only dump of what the LoRA, TN GEMM and decode-chain family WOULD launch: every hipLaunchKernelGGL in csrc/lora.hip, gemm_tn.hip
// and decode_chain.hip becomes a record in text (kernel, grid, block, dynamic LDS bytes, every argument; LoraFwdArgs, LoraDxArgs, TnArgs
// and ChainArgs field by field, all 48 L[i] included) and every entry-point call an `rc` line, over a sweep that reaches both sides of
// every host branch: both formats, the 2-D row rule at 1 / 32 / 40 / 86 column groups with M under, at and over its cap, the 1-D caps
// 16384 / 8192 / 4096 from both sides, two and three adapter slots with every admissible mask subset, accumulate, the tn rank, layout,
// output type and row-block steps, the TN GEMM's split count at 1, in between and clamped at 64 with its row floor and its reduce grid
// at 1 and at 4096, and the chain at 1 and 8 rows, three widths, 1 / 2 / 48 layers, chained and stage by stage.
// The device addresses are fake, one 2^40 range per role, never dereferenced, and printed as role+offset; `layers` of the chain is a real
// host array of such addresses. Nothing is launched and no GPU is needed. The files' anonymous namespaces clash in one unit, so build it
// once per file (-DDUMP_TU=1..3) and concatenate the outputs; two builds against two versions of the sources must print identical output
// when the host dispatch is unchanged:
//   for t in 1 2 3; do hipcc -std=c++17 -x hip --cuda-host-only -Wl,--unresolved-symbols=ignore-all -DDUMP_TU=$t \
//       -I<csrc dir to dump> -Iinclude tools/lora_chain_dispatch_dump.cpp -o dump$t; done
//   (for t in 1 2 3; do ./dump$t; done) | sha256sum
// With -Xarch_host -fsanitize=address,undefined added, the same three programs check the host loops over `layers` on the CPU.
// A kernel is named by its INSTANCE, not by the text at its launch: the launch macro hands the kernel to dump_launch as a template
// argument and the record carries its mangled name, so `<T>` inside a dispatch macro and `<bf16_t>` written out give the same record.
// Taking a kernel's address makes the host-only unit refer to a device binary that is never built: hence the linker flag.
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
#error "build with -DDUMP_TU=1 (lora.hip), 2 (gemm_tn.hip) or 3 (decode_chain.hip)"
#elif DUMP_TU == 1
#include "lora.hip"
#elif DUMP_TU == 2
#include "gemm_tn.hip"
#else
#include "decode_chain.hip"
#endif

static long n_records = 0;

// fake device addresses: role r (1..31) owns [r << 40, (r + 1) << 40); A(r) is its base, A(r, off) a byte offset into it
static char* A(unsigned long role, long off = 0) { return reinterpret_cast<char*>(role << 40) + off; }
static float* AF(unsigned long role, long off = 0) { return reinterpret_cast<float*>(A(role, off)); }

static void dump_ptr(const void* p) {
  const unsigned long a = reinterpret_cast<unsigned long>(p);
  if (!a) printf(" null");
  else if ((a >> 40) < 32) printf(" r%lu+%lu", a >> 40, a & ((1UL << 40) - 1));
  else printf(" HOST");   // a host address in a kernel argument would be a bug: make it show
}
#if DUMP_TU == 1
static void dump_arg(const LoraFwdArgs& p) {
  dump_ptr(p.qkv); printf(" %ld", p.ld_qkv);
  dump_ptr(p.tT); printf(" %ld", p.ldt);
  dump_ptr(p.Bq); dump_ptr(p.Bv); printf(" %d", p.ldb);
  dump_ptr(p.cs); dump_ptr(p.qo); dump_ptr(p.ko); dump_ptr(p.vo);
  printf(" %ld %ld %d %d %a", p.ldo, p.M, p.H, p.T, (double)p.scale);
  dump_ptr(p.Bk);
}
static void dump_arg(const LoraDxArgs& p) {
  dump_ptr(p.dtT); printf(" %ld", p.ldt);
  dump_ptr(p.A2); printf(" %ld", p.lda);
  dump_ptr(p.keep); printf(" %ld", p.ldk);
  dump_ptr(p.dx);
  printf(" %ld %ld %d %d %a", p.ldx, p.M, p.K, p.accumulate, (double)p.scale);
  dump_ptr(p.keep_v); dump_ptr(p.keep_k);
  printf(" %d", p.na);
}
#elif DUMP_TU == 2
static void dump_arg(const TnArgs& p) {
  dump_ptr(p.A); dump_ptr(p.B);
  printf(" %ld %ld %ld %d %d %ld", p.lda, p.ldb, p.M, p.N1, p.N2, p.rows_per_split);
  dump_ptr(p.part);
}
#else
static void dump_arg(const ChainArgs& p) {
  for (const ChainLayer& l : p.L)
    for (const void* q : {(const void*)l.wqkv, (const void*)l.wo, (const void*)l.wgu, (const void*)l.wd, (const void*)l.kc, (const void*)l.vc}) dump_ptr(q);
  for (const void* q : {(const void*)p.x, (const void*)p.qkv, (const void*)p.att, (const void*)p.g, (const void*)p.ssq_a, (const void*)p.ssq_b,
                        (const void*)p.ws, (const void*)p.stats0, (const void*)p.cos_sin, (const void*)p.nk_rows, (const void*)p.sync})
    dump_ptr(q);
  printf(" %d %d %d %d %d %d %a %a", p.n_layers, p.M, p.H, p.F, p.nh, p.tmax, (double)p.eps, (double)p.scale);
  for (int n : p.nb) printf(" %d", n);
  printf(" %d %d", p.per_layer, p.block0);
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

// one `rc` line per entry-point call, after the launch records the call made (if any)
static void rc(int code, const char* fmt, ...) {
  ++n_records;
  va_list ap;
  va_start(ap, fmt);
  printf("rc ");
  vprintf(fmt, ap);
  va_end(ap);
  printf(" -> %d\n", code);
}

#if DUMP_TU == 1
struct Fmt {
  const char* name;
  decltype(&haff_lora_qkv_rope_fwd) fwd;
  decltype(&haff_lora_qkv3_rope_fwd) fwd3;
  decltype(&haff_lora_qkv_rope_bwd) bwd;
  decltype(&haff_lora_dx) dx;
  decltype(&haff_lora_dx2) dx2;
  decltype(&haff_lora_dx3) dx3;
  decltype(&haff_lora_tn) tn;
  decltype(&haff_lora_out) out;
  decltype(&haff_lora_gu_swiglu) gu;
};
static const Fmt kFmts[] = {
    {"bf16", haff_lora_qkv_rope_fwd, haff_lora_qkv3_rope_fwd, haff_lora_qkv_rope_bwd, haff_lora_dx, haff_lora_dx2, haff_lora_dx3, haff_lora_tn,
     haff_lora_out, haff_lora_gu_swiglu},
    {"f16", haff_lora_qkv_rope_fwd_f16, haff_lora_qkv3_rope_fwd_f16, haff_lora_qkv_rope_bwd_f16, haff_lora_dx_f16, haff_lora_dx2_f16,
     haff_lora_dx3_f16, haff_lora_tn_f16, haff_lora_out_f16, haff_lora_gu_swiglu_f16}};

static void sweep() {
  void* const s = nullptr;
  for (const Fmt& f : kFmts) {
    // the 2-D rule: gx column groups (heads of the forward, 128-column groups of dx), ceil(M / 64) workgroup rows capped at ceil(2048 / gx)
    for (int gx : {1, 32, 40, 86}) {
      const long cap = (2048 + gx - 1) / gx;
      const int W = 128 * gx;
      for (long M : {1L, 20L, 64 * cap - 64, 64 * cap - 63, 64 * cap, 64 * cap + 1, 200 * cap}) {
        const long Mp = (M + 15) / 16 * 16;
        rc(f.fwd(A(1), 3L * W + 8, A(2, 2), Mp, A(3), A(4), 8, AF(5), A(6), A(7), A(8), W + 8, M, W, 128, 7, 0.25f, s), "%s fwd gx %d M %ld", f.name, gx, M);
        rc(f.fwd3(A(1), 3L * W, A(2), Mp + 16, A(3), A(4), A(9), 8, AF(5), A(6), A(7), A(8), W, M, W, 128, 7, 0.5f, s), "%s fwd3 gx %d M %ld", f.name, gx, M);
        for (int acc = 0; acc < 2; ++acc) {
          for (int m = 0; m < 2; ++m)               // haff_lora_dx: no mask, or its one
            rc(f.dx(A(1, 2), Mp, A(2, 2), W, m ? A(3) : nullptr, W + 8, A(4), W + 16, acc, M, W, 2.f, s), "%s dx gx %d M %ld acc %d masks %d", f.name, gx, M, acc, m);
          rc(f.dx2(A(1), Mp, A(2), W + 2, A(3), A(5), W, A(4), W, acc, M, W, 2.f, s), "%s dx2 gx %d M %ld acc %d", f.name, gx, M, acc);
          for (int m : {0, 1, 3})                   // haff_lora_dx3: none, keep_q for all, or all three
            rc(f.dx3(A(1), Mp, A(2), W, m ? A(3) : nullptr, m == 3 ? A(5) : nullptr, m == 3 ? A(6) : nullptr, W, A(4), W, acc, M, W, 2.f, s),
               "%s dx3 gx %d M %ld acc %d masks %d", f.name, gx, M, acc, m);
        }
      }
    }
    // the adjoint's 1-D grid: M * heads * 8 threads, 16384 blocks at M * heads = 2^19
    for (int nh : {1, 32})
      for (long M : {1L, 20L, (1L << 19) / nh - 32 / nh, (1L << 19) / nh, (1L << 19) / nh + 1, (1L << 22) / nh})
        rc(f.bwd(A(1), A(2), A(3), 128L * nh + 8, AF(4), A(5), 384L * nh + 16, M, 128 * nh, 128, 9, s), "%s bwd heads %d M %ld", f.name, nh, M);
    // lora_out / lora_gu_swiglu: ceil(M / 4) * (N / 8) threads, 8192 blocks at 2^21
    for (int n8 : {1, 2, 512})
      for (long M : {1L, 20L, 21L, (8191L << 10) / n8, (8192L << 10) / n8, (8192L << 10) / n8 + 1, (8192L << 12) / n8}) {
        const long M4 = (M + 3) / 4 * 4;
        rc(f.out(A(1, 8), M4, A(2), A(3), 8L * n8 + 8, M, 8 * n8, 2.f, s), "%s out N %d M %ld", f.name, 8 * n8, M);
        if (n8 > 1) rc(f.gu(A(1, 8), M4 + 4, A(2), A(3), A(4), 16L * n8 + 8, A(5), 8L * n8, M, 8 * n8, 2.f, s), "%s gu F %d M %ld", f.name, 8 * n8, M);
      }
    // tn: the rank, the layout, the output type, j_valid below R, M at the steps of lora_tn_rows_per_block, the reduce grid's cap of 4096
    for (int R : {8, 16})
      for (long M : {1L, 20L, 1024L, 1025L, 2048L, 2049L, 3072L, 3073L})
        for (int N : {2, 130, 4096})
          for (int of32 = 0; of32 < 2; ++of32)
            for (int tr = 0; tr < 2; ++tr)
              for (int jv : {R, R - 3, 1}) {
                const long ws = haff_lora_tn_workspace_elems(M, R, N);
                rc(f.tn(A(1), (M + 15) / 16 * 16, R, A(2, 4), N + 2, M, N, AF(3), ws, A(4, 2), (tr ? jv : N) + 1, of32, tr, jv, 0.5f, s),
                   "%s tn R %d M %ld N %d f32 %d tr %d jv %d ws %ld", f.name, R, M, N, of32, tr, jv, ws);
              }
    for (int N : {131040, 131072, 131074, 1 << 20})       // j_valid * N = 8 N: 4096 blocks at N = 2^17
      rc(f.tn(A(1), 32, 8, A(2), N, 20, N, AF(3), 8L * N, A(4), N, 1, 0, 8, 1.f, s), "%s tn reduce N %d", f.name, N);
  }
  for (long M : {0L, 1L, 1024L, 1025L, 2048L, 2049L, 3073L, 1L << 20})
    for (int R : {0, 8, 16})
      for (int N : {0, 130, 1 << 23}) printf("lora_tn_workspace_elems %ld %d %d -> %d\n", M, R, N, haff_lora_tn_workspace_elems(M, R, N));
}

#elif DUMP_TU == 2
static void sweep() {
  void* const s = nullptr;
  // tiles = ceil(N1 / 128) ceil(N2 / 128): want = ceil(512 / tiles) splits, clamped at 64 (1 and 8 tiles), 32 (16 tiles), 1 (1024 tiles);
  // at least 256 contraction rows per split; the reduce grid: N1 N2 / 1024 blocks, 1 at 8 x 8, 4096 at 2048 x 2048 and beyond
  const int shapes[][2] = {{8, 8}, {64, 64}, {128, 136}, {256, 512}, {512, 512}, {2048, 2048}, {2048, 2056}, {4096, 4096}};
  for (const auto& q : shapes)
    for (long M : {1L, 256L, 257L, 1000L, 16384L, 16385L, 65536L})
      for (int of32 = 0; of32 < 2; ++of32) {
        const long ws = haff_gemm_tn_workspace_elems(M, q[0], q[1]);
        rc(haff_gemm_tn_bf16(A(1), q[0] + 8, A(2), q[1] + 16, M, q[0], q[1], AF(3), ws, A(4), of32, s), "gemm_tn bf16 %d x %d M %ld f32 %d ws %ld", q[0],
           q[1], M, of32, ws);
        rc(haff_gemm_tn_f16(A(1), q[0] + 8, A(2), q[1] + 16, M, q[0], q[1], AF(3), ws, A(4), of32, s), "gemm_tn f16 %d x %d M %ld f32 %d ws %ld", q[0],
           q[1], M, of32, ws);
      }
  rc(haff_gemm_tn_bf16(A(1, 2), 64, A(2), 64, 300, 64, 64, AF(3), 8192, A(4), 0, s), "gemm_tn A off 2");
  rc(haff_gemm_tn_bf16(A(1), 64, A(2), 64, 300, 64, 64, AF(3, 8), 8192, A(4), 0, s), "gemm_tn workspace off 8");
  rc(haff_gemm_tn_f16(A(1), 64, A(2), 64, 300, 64, 64, AF(3), 8191, A(4), 1, s), "gemm_tn workspace short");
}

#else
static void sweep() {
  void* const s = nullptr;
  haff_chain_layer layers[48];
  for (int i = 0; i < 48; ++i) layers[i] = {A(1, 4096L * i), A(2, 4096L * i), A(3, 4096L * i), A(4, 4096L * i), A(5, 4096L * i), A(6, 4096L * i)};
  const int widths[][2] = {{256, 2}, {4096, 32}, {5120, 40}};
  for (int M : {1, 8})
    for (const auto& w : widths)
      for (int ffn : {256, 11008, 13824})
        for (int nl : {1, 2, 48}) {
          printf("supported %d %d %d %d %d -> %d; sync_words -> %d\n", M, w[0], ffn, w[1], nl, haff_decode_chain_supported(M, w[0], ffn, w[1], nl),
                 haff_decode_chain_sync_words(nl, w[0]));
          for (int per_stage = 0; per_stage < 2; ++per_stage)
            rc(haff_decode_chain_bf16(layers, nl, M, w[0], ffn, w[1], A(7), A(8), A(9), A(10), AF(11), AF(12), AF(13), AF(14), 1e-5f, AF(15),
                                      reinterpret_cast<int*>(A(16)), 299, 0.088f, reinterpret_cast<unsigned*>(A(17)), per_stage, s),
               "chain M %d hidden %d ffn %d heads %d layers %d per_stage %d", M, w[0], ffn, w[1], nl, per_stage);
        }
  // the refusals that read `layers`: a null and a misaligned member in the first and in the last layer
  for (int at : {0, 47})
    for (int how = 0; how < 2; ++how) {
      haff_chain_layer saved = layers[at];
      if (how) layers[at].vcache = A(6, 8); else layers[at].wo = nullptr;
      rc(haff_decode_chain_bf16(layers, 48, 2, 256, 256, 2, A(7), A(8), A(9), A(10), AF(11), AF(12), AF(13), AF(14), 1e-5f, AF(15),
                                reinterpret_cast<int*>(A(16)), 299, 0.088f, reinterpret_cast<unsigned*>(A(17)), 0, s),
         "chain layer %d %s", at, how ? "vcache off 8" : "wo null");
      layers[at] = saved;
    }
  rc(haff_decode_chain_status(nullptr, 2, s), "status null sync");
  rc(haff_decode_chain_status(reinterpret_cast<unsigned*>(A(17)), 49, s), "status 49 layers");
}
#endif

int main() {
  sweep();
  fprintf(stderr, "%ld records\n", n_records);
  return 0;
}
