// Host-only dump of what csrc/gemm_nf4.hip and csrc/gemm_int8.hip WOULD launch: every hipLaunchKernelGGL becomes a record in text
// (the kernel instance, the launching function and its template arguments, grid, block, every argument; an argument block field by
// field), over a sweep of all nine entry points, together with every return code. Nothing is launched and no GPU is needed. Two
// builds of this file against two versions of the sources must print identical output when the host dispatch is unchanged:
//   hipcc -std=c++17 -x hip --cuda-host-only -I<dir with the gemm_nf4.hip and gemm_int8.hip to dump> -Iinclude tools/quant_dispatch_dump.cpp -o dump && ./dump | sha256sum
// The kernel is printed as the compiler resolves it at the launch (the demangled instance, gemm_nf4_kernel<2, 2, false, 8, true>(...),
// not the launch's source text): renaming a constant in a template argument list leaves the record alone, a different instance, and
// with it a different mangled kernel name, does not.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cxxabi.h>
#include <type_traits>
#include <typeinfo>
#undef hipLaunchKernelGGL
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) dump_launch<kernel>(__func__, __PRETTY_FUNCTION__, grid, block, __VA_ARGS__)
#define hipGetLastError() hipSuccess
template <auto Kernel, typename... Args> static void dump_launch(const char* fn, const char* pretty, dim3 g, dim3 b, const Args&... args);
#include "gemm_nf4.hip"
#include "gemm_int8.hip"

static long n_records = 0;
template <auto Kernel> struct KernelTag {};

static void dump_arg(const void* p) { printf(" %p", p); }
template <typename T> static std::enable_if_t<std::is_integral_v<T>> dump_arg(T v) { printf(" %ld", (long)v); }
static void dump_arg(float v) { printf(" %a", (double)v); }
static void dump_arg(const Nf4Args& p) {
  printf("\n A %p lda %ld Wq %p absmax %p C %p ldc %ld bias %p resid %p ldr %ld row_map %p M %d N %d K %d act %d out_f32 %d", (const void*)p.A,
         p.lda, (const void*)p.Wq, (const void*)p.absmax, p.C, p.ldc, (const void*)p.bias, p.resid, p.ldr, (const void*)p.row_map, p.M, p.N, p.K,
         p.act, p.out_f32);
}
static void dump_arg(const Nf4LoraArgs& p) {
  dump_arg(static_cast<const Nf4Args&>(p));
  printf("\n t %p ldt %ld B %p nseg %d seg_rows %d scale %a", (const void*)p.t, p.ldt, (const void*)p.B, p.nseg, p.seg_rows, (double)p.scale);
}
static void dump_arg(const I8Args& p) {
  printf("\n A %p lda %ld CA %p ldca %ld SCA %p CB %p SCB %p cols %p ncols %p seg_rows %d", (const void*)p.A, p.lda, (const void*)p.CA, p.ldca,
         (const void*)p.SCA, (const void*)p.CB, (const void*)p.SCB, (const void*)p.cols, (const void*)p.ncols, p.seg_rows);
  printf("\n C %p ldc %ld bias %p resid %p ldr %ld row_map %p M %d N %d K %d act %d out_f32 %d", p.C, p.ldc, (const void*)p.bias, p.resid, p.ldr,
         (const void*)p.row_map, p.M, p.N, p.K, p.act, p.out_f32);
}

template <auto Kernel, typename... Args> static void dump_launch(const char* fn, const char* pretty, dim3 g, dim3 b, const Args&... args) {
  ++n_records;
  int status = 0;
  char* tag = abi::__cxa_demangle(typeid(KernelTag<Kernel>).name(), nullptr, nullptr, &status);   // "KernelTag<&name<...>(...)>"
  const char* targs = strchr(pretty, '[');                                                        // the launching function's template arguments
  printf("%s in %s %s grid %u %u %u block %u %u %u :", tag ? tag : typeid(KernelTag<Kernel>).name(), fn, targs ? targs : "", g.x, g.y, g.z, b.x,
         b.y, b.z);
  free(tag);
  (dump_arg(args), ...);
  printf("\n");
}

// fake device addresses (never dereferenced), one per role
static void* at(unsigned long a) { return reinterpret_cast<void*>(a << 20); }
static void *A = at(1), *WQ = at(2), *C = at(3), *RES = at(5), *T = at(7), *LB = at(8), *ACAT = at(9), *W16 = at(10), *WS = at(11), *CA = at(13),
            *CB = at(14);
static float *BIAS = (float*)at(4), *AMAX = (float*)at(12), *OFF = (float*)at(15), *SCA = (float*)at(16), *SCB = (float*)at(17);
static int *RMAP = (int*)at(6), *COLS = (int*)at(18), *NCOLS = (int*)at(19), *VALID = (int*)at(20);
static unsigned* MASKS = (unsigned*)at(21);

struct Epi { const float* bias; const void* resid; const int* row_map; int act, out_f32; };
static const Epi kEpis[] = {{nullptr, nullptr, nullptr, 0, 0}, {BIAS, RES, RMAP, HAFF_ACT_SILU, 1}};

static void products(int M, int N, int K) {
  for (int swiglu = 0; swiglu < 2; ++swiglu)
    for (const Epi& e : kEpis) {
      const void* resid = swiglu ? nullptr : e.resid;     // SwiGLU takes no residual
      const long ldc = swiglu ? N / 2 : N;
      printf("rc nf4 %d %d %d swiglu=%d -> %d\n", M, N, K, swiglu,
             haff_gemm_nf4_f16(A, K, WQ, AMAX, C, ldc, e.bias, resid, ldc, e.row_map, M, N, K, e.act, e.out_f32, swiglu, nullptr));
      for (int nseg = 1; nseg <= 3; nseg += 2)
        printf("rc nf4_lora %d %d %d swiglu=%d nseg=%d -> %d\n", M, N, K, swiglu, nseg,
               haff_gemm_nf4_lora_f16(A, K, WQ, AMAX, C, ldc, e.bias, resid, ldc, e.row_map, M, N, K, e.act, e.out_f32, swiglu, T, 8 * nseg, LB,
                                      nseg, nseg == 1 ? 16 : 4096, 2.0f, nullptr));
      for (int form = 0; form <= 2; ++form)
        for (int outliers = 0; outliers < 2; ++outliers)
          printf("rc int8 %d %d %d swiglu=%d form=%d outliers=%d -> %d\n", M, N, K, swiglu, form, outliers,
                 haff_gemm_int8_f16(A, K, CA, K, SCA, CB, SCB, outliers ? COLS : nullptr, outliers ? NCOLS : nullptr, M > 16 ? 16 : 1, C, ldc,
                                    e.bias, resid, ldc, e.row_map, M, N, K, e.act, e.out_f32, swiglu, form, nullptr));
    }
}

static void weights(int N, int K) {
  const long np = (N + 7) & ~7L;
  for (int mapped = 0; mapped < 2; ++mapped) {
    const int* rm = mapped ? RMAP : nullptr;
    for (int dq = 0; dq < 2; ++dq)
      printf("rc nf4_quantize %d %d dq=%d -> %d\n", N, K, dq, haff_nf4_quantize_f16(W16, K, N, K, dq, rm, WQ, AMAX, OFF, WS, 4L * N * (K / 64), nullptr));
    printf("rc nf4_dequant %d %d -> %d\n", N, K, haff_nf4_dequant_f16(WQ, AMAX, N, K, rm, W16, K + 8, nullptr));
    printf("rc nf4_dequant_t %d %d -> %d\n", N, K, haff_nf4_dequant_t_f16(WQ, AMAX, N, K, rm, W16, np, nullptr));
    for (int nseg = 1; nseg <= 3; ++nseg)
      printf("rc nf4_dequant_lora %d %d nseg=%d -> %d\n", N, K, nseg,
             haff_nf4_dequant_lora_f16(WQ, AMAX, N, K, rm, W16, K, ACAT, K, LB, nseg, nseg == 2 ? 16 : 4096, 0.25f, nullptr));
    printf("rc int8_weight %d %d -> %d\n", N, K, haff_int8_quantize_weight_f16(W16, K, N, K, rm, CB, SCB, nullptr));
  }
}

static void rows(int M, int K) {
  for (int seg_rows : {1, 3, M})
    for (float thr : {0.f, 6.f})
      for (int masks = 0; masks < 2; ++masks)            // (a positive threshold without masks is refused: the code is part of the record)
        for (int valid = 0; valid < 2; ++valid)
          printf("rc int8_act %d %d seg_rows=%d thr=%g masks=%d valid=%d -> %d\n", M, K, seg_rows, (double)thr, masks, valid,
                 haff_int8_quantize_act_f16(A, K, M, K, thr, seg_rows, valid ? VALID : nullptr, masks ? MASKS : nullptr, CA, K, SCA, COLS, NCOLS,
                                            nullptr));
}

int main() {
  const int Ms[] = {1, 16, 17, 32, 33, 64, 65, 129};
  const int Ns[] = {64, 4096, 6128, 6144, 12288, 32003};   // 6128 / 6144: 191 / 192 pairs of 16-row tiles, either side of the raster rule
  const int Ks[] = {64, 4096, 11008};
  for (int M : Ms)
    for (int N : Ns)
      for (int K : Ks) products(M, N, K);
  for (int N : Ns)
    for (int K : Ks) weights(N, K);
  for (int M : {1, 17, 64, 291})
    for (int K : {64, 4096, 32768, 32832}) rows(M, K);       // K / 32 = 1024 and 1026: either side of kI8RowMaxWords
  fprintf(stderr, "%ld launch records\n", n_records);
  return 0;
}
