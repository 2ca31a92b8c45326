// Host-only dump of what csrc/gemm_bf16.hip WOULD launch: every hipLaunchKernelGGL becomes a record in text (the kernel instance as
// written at the launch plus the launching function's template arguments, grid, block, every GemmArgs field), over a sweep of all
// its entry points. Nothing is launched and no GPU is needed. Two builds of
// this file against two versions of gemm_bf16.hip must print identical output when the host dispatch is unchanged:
//   hipcc -std=c++17 -x hip --cuda-host-only -I<dir with the gemm_bf16.hip to dump> -Iinclude tools/gemm_dispatch_dump.cpp -o dump && ./dump | sha256sum
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstring>
#undef hipLaunchKernelGGL
#define DUMP_STR(...) #__VA_ARGS__
#define hipLaunchKernelGGL(kernel, grid, block, shmem, stream, ...) \
  dump_launch(DUMP_STR(kernel), __func__, __PRETTY_FUNCTION__, grid, block, __VA_ARGS__)
#define hipGetLastError() hipSuccess
template <typename Args> static void dump_launch(const char* kernel, const char* fn, const char* pretty, dim3 g, dim3 b, const Args& p);
#include "gemm_bf16.hip"

static long n_records = 0;
template <typename Args> static void dump_launch(const char* kernel, const char* fn, const char* pretty, dim3 g, dim3 b, const Args& p) {
  ++n_records;
  const char* targs = strchr(pretty, '[');   // the launching function's template arguments resolve the names in the kernel's text
  printf("%s in %s %s grid %u %u %u block %u %u %u\n", kernel, fn, targs ? targs : "", g.x, g.y, g.z, b.x, b.y, b.z);
  printf(" A %p lda %ld W %p ldw %ld C %p ldc %ld bias %p resid %p ldr %ld row_map %p a_map %p group_m %d ln_stats %p ln_colsum %p\n",
         (const void*)p.A, p.lda, (const void*)p.W, p.ldw, p.C, p.ldc, (const void*)p.bias, p.resid, p.ldr, (const void*)p.row_map,
         (const void*)p.a_map, p.group_m, (const void*)p.ln_stats, (const void*)p.ln_colsum);
  printf(" M %d N %d K %d act %d out_f32 %d swiglu %d nb_inner %d sA %ld %ld sW %ld %ld sC %ld %ld deep_k %d k_total %d nt_out %d ws %p ksplit %d\n",
         p.M, p.N, p.K, p.act, p.out_f32, p.swiglu, p.nb_inner, p.sAo, p.sAi, p.sWo, p.sWi, p.sCo, p.sCi, p.deep_k, p.k_total, p.nt_out,
         (const void*)p.ws, p.ksplit);
  printf(" ssq_out %p ssq_in %p ssq_n %d ssq_eps %a stat_out %p stat_slots %d res32 %p ld32 %ld rope_cs %p rope_k %p rope_v %p rope %d %d %d %d"
         " hm %d %d %ld %ld\n", (const void*)p.ssq_out, (const void*)p.ssq_in, p.ssq_n, (double)p.ssq_eps, (const void*)p.stat_out, p.stat_slots,
         (const void*)p.res32, p.ld32, (const void*)p.rope_cs, p.rope_k, p.rope_v, p.rope_t, p.rope_tmax, p.rope_pos0, p.rope_hd, p.hm_d,
         p.hm_hd, p.hm_part, p.hm_head);
}

// fake device addresses (never dereferenced), one per role
static void* at(unsigned long a) { return reinterpret_cast<void*>(a << 20); }
static void *A = at(1), *W = at(2), *C = at(3), *RES = at(5), *WS = at(12), *KC = at(13), *VC = at(14);
static float *BIAS = (float*)at(4), *LN = (float*)at(8), *CSUM = (float*)at(9), *SSQI = (float*)at(10), *SSQO = (float*)at(11),
             *CS = (float*)at(15), *STAT = (float*)at(16), *X32 = (float*)at(17);
static int *RMAP = (int*)at(6), *AMAP = (int*)at(7);
static const long WS_BYTES = 256L << 20;

template <bool F16> static void general(int M, int N, int K) {
  auto rc = [&](const char* what, int r) { printf("rc %s %d %d %d f16=%d -> %d\n", what, M, N, K, (int)F16, r); };
  const long lda = K, ldw = K, ldc = N;
  struct Epi { const float* bias; const void* resid; const int* row_map; int act, out_f32, swiglu; };
  const Epi epis[] = {{nullptr, nullptr, nullptr, 0, 0, 0}, {BIAS, nullptr, nullptr, 0, 0, 0}, {nullptr, RES, nullptr, 0, 0, 0},
                      {BIAS, RES, nullptr, 0, 0, 0}, {nullptr, nullptr, nullptr, 0, 0, 1}, {BIAS, nullptr, nullptr, HAFF_ACT_QUICK_GELU, 0, 0},
                      {BIAS, nullptr, nullptr, HAFF_ACT_GELU, 0, 0}, {nullptr, nullptr, nullptr, 0, 1, 0}, {BIAS, nullptr, RMAP, 0, 0, 0},
                      {nullptr, RES, nullptr, HAFF_ACT_SILU, 1, 0}, {BIAS, nullptr, nullptr, 0, 1, 1}};
  auto gemm = F16 ? haff_gemm_f16 : haff_gemm_bf16;
  auto ws = F16 ? haff_gemm_f16_ws : haff_gemm_bf16_ws;
  auto cfg = F16 ? haff_gemm_f16_cfg : haff_gemm_bf16_cfg;
  auto gather = F16 ? haff_gemm_f16_gather : haff_gemm_bf16_gather;
  auto ln = F16 ? haff_gemm_f16_ln : haff_gemm_bf16_ln;
  for (const Epi& e : epis) {
    const long ldo = e.swiglu ? N / 2 : N;
    rc("gemm", gemm(A, lda, W, ldw, C, ldo, e.bias, e.resid, ldc, e.row_map, M, N, K, e.act, e.out_f32, e.swiglu, nullptr));
    rc("ws", ws(A, lda, W, ldw, C, ldo, e.bias, e.resid, ldc, e.row_map, M, N, K, e.act, e.out_f32, e.swiglu, WS, WS_BYTES, nullptr));
    for (int t = 1; t <= 3; ++t)
      rc("cfg", cfg(A, lda, W, ldw, C, ldo, e.bias, e.resid, ldc, e.row_map, M, N, K, e.act, e.out_f32, e.swiglu, t, nullptr));
    rc("gather", gather(A, lda, AMAP, M + 7, W, ldw, C, ldo, e.bias, e.resid, ldc, e.row_map, M, N, K, e.act, e.out_f32, e.swiglu, nullptr));
    rc("ln", ln(A, lda, W, ldw, C, ldo, e.bias, e.resid, ldc, e.row_map, LN, CSUM, M, N, K, e.act, e.out_f32, e.swiglu, nullptr));
    rc("rmsfold", ln(A, lda, W, ldw, C, ldo, e.bias, e.resid, ldc, e.row_map, LN, nullptr, M, N, K, e.act, e.out_f32, e.swiglu, nullptr));
  }
  if (M <= 16 && K % 128 == 0) {   // the RMSNorm-carrying decode products: consumer, producer, both, SwiGLU consumer
    int parts = -1;
    auto rms = F16 ? haff_gemm_f16_rms : haff_gemm_bf16_rms;
    rc("rms", rms(A, lda, W, ldw, C, ldc, nullptr, nullptr, 0, M, N, K, 0, 0, 0, M <= 8 ? SSQI : nullptr, 256, 1e-5f, nullptr, &parts, nullptr));
    rc("rms", rms(A, lda, W, ldw, C, ldc, BIAS, RES, ldc, M, N, K, 0, 0, 0, nullptr, 0, 0.f, SSQO, &parts, nullptr));
    rc("rms", rms(A, lda, W, ldw, C, N / 2, nullptr, nullptr, 0, M, N, K, 0, 0, 1, M <= 8 ? SSQI : nullptr, 512, 1e-6f, nullptr, &parts, nullptr));
    printf("parts %d\n", parts);
  }
  if (M % 256 == 0) {   // whole-tile entry points (they refuse the other shapes: the code is part of the record)
    auto rs = F16 ? haff_gemm_f16_rowstats : haff_gemm_bf16_rowstats;
    rc("rowstats", rs(A, lda, nullptr, 0, W, ldw, C, ldc, BIAS, RES, ldc, M, N, K, STAT, nullptr));
    rc("rowstats", rs(A, lda, AMAP, M + 7, W, ldw, C, ldc, nullptr, RES, ldc, M, N, K, STAT, nullptr));
    if (!F16) rc("rowstats32", haff_gemm_bf16_rowstats32(A, lda, nullptr, 0, W, ldw, X32, ldc, C, ldc, BIAS, M, N, K, STAT, nullptr));
    if (!F16) rc("rowstats32", haff_gemm_bf16_rowstats32(A, lda, AMAP, M + 7, W, ldw, X32, ldc, C, ldc, BIAS, M, N, K, STAT, nullptr));
    auto hm = F16 ? haff_gemm_f16_heads : haff_gemm_bf16_heads;
    for (int d : {64, 80, 128})
      for (int parts : {1, 3}) {
        if (N % (parts * d)) continue;
        const int heads = N / (parts * d);
        rc("heads", hm(A, lda, W, ldw, C, BIAS, RMAP, LN, CSUM, M, N, K, d, heads, (long)(M + 256) * heads * d, 200L * d, nullptr));
        rc("heads", hm(A, lda, W, ldw, C, nullptr, RMAP, nullptr, nullptr, M, N, K, d, heads, (long)(M + 256) * heads * d, 200L * d, nullptr));
      }
  }
  auto bt = F16 ? haff_gemm_f16_batched : haff_gemm_bf16_batched;
  if ((long)M * N <= (1L << 22))
    for (int nbo : {1, 4, 64})
      for (int nbi : {1, 16})
        for (int f32 : {0, 1})
          rc("batched", bt(A, lda, (long)M * K * nbi, (long)M * K, W, ldw, (long)N * K * nbi, (long)N * K, C, ldc, (long)M * N * nbi, (long)M * N, nbo, nbi, M, N, K, f32, nullptr));
}

template <bool F16> static void qkv_rope() {
  auto f = F16 ? haff_gemm_f16_qkv_rope : haff_gemm_bf16_qkv_rope;
  for (int H : {2, 32, 40})
    for (int K : {64, 4096, 5120})
      for (int B : {1, 4, 64})
        for (int T : {1, 16, 291, 1000})
          printf("rc qkv_rope %d %d %d %d f16=%d -> %d\n", H, K, B, T, (int)F16,
                 f(A, K, W, K, C, H * 128, KC, VC, CS, B, T, 1024, 24, H, 128, K, nullptr));
}

int main() {
  const int Ms[] = {1, 8, 16, 17, 32, 33, 64, 65, 128, 255, 256, 257, 1024, 2808, 4096, 18624};
  const int Ns[] = {256, 1024, 4096, 8192, 11008 * 2, 16384, 32000};
  const int Ks[] = {64, 128, 1024, 4096, 5120, 11008};
  // the workload's own products: ViT-H (32 frames), Llama 7B / 13B prefill at 64 x 291 rows and decode at 64, the 2808-row fine-tune
  // step, CLIP at 1 and 64 frames
  const int own[][3] = {{131072, 3840, 1280}, {131072, 1280, 1280}, {131072, 5120, 1280}, {131072, 1280, 5120}, {18624, 12288, 4096},
                        {18624, 4096, 4096}, {18624, 22016, 4096}, {18624, 4096, 11008}, {18624, 15360, 5120}, {18624, 5120, 5120},
                        {18624, 27648, 5120}, {18624, 5120, 13824}, {64, 12288, 4096}, {64, 27648, 5120}, {64, 5120, 13824}, {64, 32003, 4096},
                        {2808, 12288, 4096}, {2808, 4096, 22016}, {2808, 22016, 4096}, {2808, 32003, 4096}, {257, 3072, 1024}, {257, 1024, 1024},
                        {257, 4096, 1024}, {257, 1024, 4096}, {16448, 3072, 1024}, {16448, 1024, 1024}, {16448, 4096, 1024}, {16448, 1024, 4096},
                        {288, 4096, 4096}, {5000, 4096, 4096}, {100, 200, 72},
                        {1048576, 1024, 2048}, {1024, 1048576, 2048}};   // an operand of 4 GiB: no 8-wave tile
  for (int pass = 0; pass < 2; ++pass) {   // second pass: the stream capped to 224 workgroups (a short sweep)
    if (pass) haff_gemm_stream_cap(nullptr, 224);
    for (int M : Ms)
      for (int N : Ns)
        for (int K : Ks) {
          if (pass && !(M >= 256 && K == 1024)) continue;
          general<false>(M, N, K);
          general<true>(M, N, K);
        }
    for (const auto& s : own) {
      general<false>(s[0], s[1], s[2]);
      general<true>(s[0], s[1], s[2]);
    }
    qkv_rope<false>();
    qkv_rope<true>();
  }
  fprintf(stderr, "%ld launch records\n", n_records);
  return 0;
}
