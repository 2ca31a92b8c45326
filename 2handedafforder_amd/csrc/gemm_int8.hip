// LLM.int8 language-model weights for the fp16 inference mode (load_in_8bit): the load-time weight quantiser, the activation
// quantiser with per-frame outlier columns, and the int8 product on the int8 matrix cores (v_mfma_i32_16x16x64_i8).
//
// The format and the arithmetic are the ones bitsandbytes' `load_in_8bit=True` (llm_int8_threshold 6.0, no fp16 weight copy)
// gives the reference (2Haff/inference.py:147-156), restated in 2handedafforder_amd/quant.py:
//   CB   int8 [N][K]  rint(w * (127 / SCB[n])), SCB[n] = fp32 max |W[n][:]|        (row-local: row reorders stay row reorders)
//   CA   int8 [M][K]  rint(a * (127 / SCA[m])), 0 on the outlier columns of row m's segment and on row m's own outliers
//   SCA  fp32 [M]     max |a| over row m's non-outlier elements (|a| < threshold)
// Y[m][n] = f16(f32(CA[m] . CB[n]) * C * SCA[m] * SCB[n] + bias[n]), left to right and not contracted (C = 6.200012e-05f), then,
// when row m's segment has outlier columns, Y = f16(Y + f16(sum over those columns, ascending, of a[m][c] * subB[n][c])) with
// subB[n][c] = f16(f32(CB[n][c]) * SCB[n] / 127). The int32 accumulation is exact and the outlier sum has a fixed order, so
// a row's output depends on nothing but that row, its segment's columns and the weights: bit-identical whatever M, batch
// composition or kernel form.
//
// Segments: rows [s * seg_rows, (s + 1) * seg_rows) are segment s (one frame); only its first seg_valid[s] rows (NULL: all) put
// outlier columns into its mask. The masks (uint32 [S][K/32]) are ORed into, never cleared here: the caller zeroes them for a
// fresh call and keeps them across a frame's decode steps (sticky masks: a decode row sees the whole prefix's columns).
#include "haff_common.h"
#include "gemm_quant.h"

#pragma clang fp contract(off)

namespace {

typedef __attribute__((ext_vector_type(4))) int i32x4;

constexpr float kI8C = 6.200012e-05f;   // bitsandbytes' dequantisation constant (~1 / 127^2)

__device__ __forceinline__ float f16r(float x) { return (float)(f16_t)x; }

__device__ __forceinline__ i32x4 mfma_i8(uint4 a, uint4 b, i32x4 c) {
  return __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, a), __builtin_bit_cast(i32x4, b), c, 0, 0, 0);
}

__device__ __forceinline__ float block_max256(float v, float* red) {
  v = wave_max(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  v = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
  __syncthreads();
  return v;
}

// Weight quantiser: workgroup = one source row n -> row map[n] (or n) of CB / SCB
__global__ __launch_bounds__(256) void i8_weight_kernel(const f16_t* __restrict__ W, long ldw, int K, const int* row_map,
                                                        signed char* __restrict__ CB, float* __restrict__ SCB) {
  __shared__ float red[4];
  const int n = blockIdx.x;
  const f16_t* w = W + (long)n * ldw;
  float a = 0.f;
  for (int k = 8 * threadIdx.x; k < K; k += 8 * 256) {
    float v[8];
    load8(w + k, v);
#pragma unroll
    for (int i = 0; i < 8; ++i) a = fmaxf(a, fabsf(v[i]));
  }
  a = block_max256(a, red);
  const float s = a > 0.f ? __fdiv_rn(127.0f, a) : 0.f;
  const long dst = row_map ? row_map[n] : n;
  signed char* cb = CB + dst * K;
  for (int k = 8 * threadIdx.x; k < K; k += 8 * 256) {
    float v[8];
    load8(w + k, v);
    unsigned lo = 0, hi = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      lo |= ((unsigned)(int)rintf(__fmul_rn(v[i], s)) & 0xffu) << (8 * i);
      hi |= ((unsigned)(int)rintf(__fmul_rn(v[i + 4], s)) & 0xffu) << (8 * i);
    }
    *reinterpret_cast<uint2*>(cb + k) = uint2{lo, hi};
  }
  if (threadIdx.x == 0) SCB[dst] = a;
}

// 32 consecutive f16 of a row (word w of its mask)
__device__ __forceinline__ void load32(const f16_t* p, float (&v)[32]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float t[8];
    load8(p + 8 * i, t);
#pragma unroll
    for (int j = 0; j < 8; ++j) v[8 * i + j] = t[j];
  }
}

// The three steps of the activation quantiser on one row / one segment; `mask` is the segment's mask words (global or LDS).
// Scan: SCA = max |a| of the non-outliers; a valid row ORs its outlier columns into the mask (bitwise OR: the result does not
// depend on the order of the rows; `shared` masks belong to one workgroup and take a plain OR)
template <bool SHARED>
__device__ __forceinline__ float act_scan_row(const f16_t* a, int kw, float thr, bool valid, unsigned* mask, float* red) {
  float mx = 0.f;
  for (int w = threadIdx.x; w < kw; w += 256) {
    float v[32];
    load32(a + 32 * w, v);
    unsigned bits = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      const float x = fabsf(v[i]);
      const bool out = thr > 0.f && x >= thr;
      bits |= (unsigned)out << i;
      if (!out) mx = fmaxf(mx, x);
    }
    if (bits && valid) {
      if constexpr (SHARED) mask[w] |= bits; else atomicOr(mask + w, bits);
    }
  }
  return block_max256(mx, red);
}

// Codes rint(a * (127 / SCA)), 0 on the segment's columns and the row's own outliers
__device__ __forceinline__ void act_codes_row(const f16_t* a, int kw, float thr, const unsigned* mask, float sca, signed char* ca) {
  const float sc = sca > 0.f ? __fdiv_rn(127.0f, sca) : 0.f;
  for (int w = threadIdx.x; w < kw; w += 256) {
    float v[32];
    load32(a + 32 * w, v);
    const unsigned mb = mask ? mask[w] : 0u;
    unsigned q[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      unsigned word = 0;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float x = v[4 * j + i];
        const bool out = ((mb >> (4 * j + i)) & 1u) || (thr > 0.f && fabsf(x) >= thr);
        const int c = out ? 0 : (int)rintf(__fmul_rn(x, sc));
        word |= ((unsigned)c & 0xffu) << (8 * i);
      }
      q[j] = word;
    }
    uint4* dst = reinterpret_cast<uint4*>(ca + 32 * w);
    dst[0] = uint4{q[0], q[1], q[2], q[3]};
    dst[1] = uint4{q[4], q[5], q[6], q[7]};
  }
}

// A segment's mask as an ascending column list cols[0 .. *ncols)
__device__ __forceinline__ void act_cols_seg(const unsigned* mask, int kw, int* cols, int* ncols, int* part) {
  int base = 0;
  for (int w0 = 0; w0 < kw; w0 += 256) {
    const int w = w0 + threadIdx.x;
    const unsigned mb = (mask && w < kw) ? mask[w] : 0u;
    const int cnt = __popc(mb);
    part[threadIdx.x] = cnt;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {    // inclusive scan (Hillis-Steele)
      const int v = (int)threadIdx.x >= o ? part[threadIdx.x - o] : 0;
      __syncthreads();
      part[threadIdx.x] += v;
      __syncthreads();
    }
    int pos = base + part[threadIdx.x] - cnt;
    unsigned b = mb;
    while (b) {
      const int i = __ffs(b) - 1;
      cols[pos++] = 32 * w + i;
      b &= b - 1;
    }
    base += part[255];
    __syncthreads();
  }
  if (threadIdx.x == 0) *ncols = base;
}

// Pass 1: workgroup = row m
__global__ __launch_bounds__(256) void i8_act_scan_kernel(const f16_t* __restrict__ A, long lda, int K, float thr, int seg_rows,
                                                          const int* seg_valid, unsigned* masks, float* __restrict__ SCA) {
  __shared__ float red[4];
  const int m = blockIdx.x, s = m / seg_rows, kw = K >> 5;
  const bool valid = !seg_valid || (m - s * seg_rows) < seg_valid[s];
  const float mx = act_scan_row<false>(A + (long)m * lda, kw, thr, valid, masks ? masks + (long)s * kw : nullptr, red);
  if (threadIdx.x == 0) SCA[m] = mx;
}

// Pass 2: workgroup = row m
__global__ __launch_bounds__(256) void i8_act_codes_kernel(const f16_t* __restrict__ A, long lda, int K, float thr, int seg_rows,
                                                           const unsigned* masks, const float* __restrict__ SCA,
                                                           signed char* __restrict__ CA, long ldca) {
  const int m = blockIdx.x, s = m / seg_rows, kw = K >> 5;
  act_codes_row(A + (long)m * lda, kw, thr, masks ? masks + (long)s * kw : nullptr, SCA[m], CA + (long)m * ldca);
}

// Pass 3: workgroup = segment s
__global__ __launch_bounds__(256) void i8_act_cols_kernel(const unsigned* masks, int K, int* __restrict__ cols, int* __restrict__ ncols) {
  __shared__ int part[256];
  const int s = blockIdx.x, kw = K >> 5;
  act_cols_seg(masks ? masks + (long)s * kw : nullptr, kw, cols + (long)s * K, ncols + s, part);
}

// One-row segments (every decode step, lm_head on the last rows): workgroup = row m = segment m, the three steps in ONE launch on an
// LDS copy of the row's mask (no other workgroup touches it), the mask written back once
constexpr int kI8RowMaxWords = 1024;   // K <= 32768
__global__ __launch_bounds__(256) void i8_act_row_kernel(const f16_t* __restrict__ A, long lda, int K, float thr, const int* seg_valid,
                                                         unsigned* masks, float* __restrict__ SCA, signed char* __restrict__ CA,
                                                         long ldca, int* __restrict__ cols, int* __restrict__ ncols) {
  __shared__ unsigned smask[kI8RowMaxWords];
  __shared__ float red[4];
  __shared__ int part[256];
  const int m = blockIdx.x, kw = K >> 5;
  const bool valid = !seg_valid || seg_valid[m] > 0;
  unsigned* gm = masks ? masks + (long)m * kw : nullptr;
  for (int w = threadIdx.x; w < kw; w += 256) smask[w] = gm ? gm[w] : 0u;
  __syncthreads();
  const f16_t* a = A + (long)m * lda;
  const float sca = act_scan_row<true>(a, kw, thr, valid, smask, red);   // (ends in a barrier: smask is complete)
  if (threadIdx.x == 0) SCA[m] = sca;
  if (gm)
    for (int w = threadIdx.x; w < kw; w += 256) gm[w] = smask[w];
  act_codes_row(a, kw, thr, gm ? smask : nullptr, sca, CA + (long)m * ldca);
  act_cols_seg(gm ? smask : nullptr, kw, cols + (long)m * K, ncols + m, part);
}

struct I8Args {
  const f16_t* A; long lda;                 // the f16 input rows (outlier values)
  const signed char* CA; long ldca; const float* SCA;
  const signed char* CB; const float* SCB;  // CB row stride K
  const int* cols; const int* ncols; int seg_rows;
  void* C; long ldc;
  const float* bias;
  const void* resid; long ldr;
  const int* row_map;
  int M, N, K, act, out_f32;
};

// Y of one output (f16-valued): the dequantisation, then the outlier add of the row's segment columns
__device__ __forceinline__ float i8_y(const I8Args& p, int m, int n, int acc, int nc, const int* cl) {
  float t = (float)acc;
  t = t * kI8C;
  t = t * p.SCA[m];
  t = t * p.SCB[n];
  if (p.bias) t = t + p.bias[n];
  float y = f16r(t);
  if (nc > 0) {
    const float sb = p.SCB[n];
    const signed char* wr = p.CB + (long)n * p.K;
    const f16_t* ar = p.A + (long)m * p.lda;
    float s = 0.f;
    for (int j = 0; j < nc; ++j) {
      const int c = cl[j];
      const float b = f16r(__fdiv_rn((float)wr[c] * sb, 127.0f));
      s = s + (float)ar[c] * b;     // f16 x f16 is exact in fp32
    }
    y = f16r(y + f16r(s));
  }
  return y;
}

// The epilogue of one lane: row m, the 4 outputs 4 fh + r of the 16-row weight tile starting at nt (SwiGLU: the gate tile at nt,
// the up tile at nt + 16, outputs nt / 2 + 4 fh + r). After Y: act or SwiGLU, residual (may alias C), row map, f16 / f32 out.
template <bool SWIGLU>
__device__ __forceinline__ void i8_epilogue(const I8Args& p, int m, int nt, int fh, const i32x4& a0, const i32x4& a1) {
  if (m >= p.M || nt >= p.N) return;
  long orow = m;
  if (p.row_map) {
    orow = p.row_map[m];
    if (orow < 0) return;
  }
  const int seg = m / p.seg_rows;
  const int nc = p.ncols ? p.ncols[seg] : 0;
  const int* cl = p.cols ? p.cols + (long)seg * p.K : nullptr;
  const int n_out = SWIGLU ? (p.N >> 1) : p.N;
  const int nb = (SWIGLU ? (nt >> 1) : nt) + 4 * fh;
  float val[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    val[r] = 0.f;
    if (nb + r >= n_out) continue;
    if constexpr (SWIGLU) {
      const int ng = nt + 4 * fh + r;
      const float g = i8_y(p, m, ng, a0[r], nc, cl);
      const float u = i8_y(p, m, ng + 16, a1[r], nc, cl);
      val[r] = g * __builtin_amdgcn_rcpf(1.0f + __expf(-g)) * u;
    } else {
      val[r] = apply_act(i8_y(p, m, nt + 4 * fh + r, a0[r], nc, cl), p.act);
    }
  }
  if (p.out_f32) {
    float* c = reinterpret_cast<float*>(p.C) + orow * p.ldc + nb;
    const float* rs = p.resid ? reinterpret_cast<const float*>(p.resid) + orow * p.ldr + nb : nullptr;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (nb + r < n_out) c[r] = val[r] + (rs ? rs[r] : 0.f);
  } else {
    f16_t* c = reinterpret_cast<f16_t*>(p.C) + orow * p.ldc + nb;
    const f16_t* rs = p.resid ? reinterpret_cast<const f16_t*>(p.resid) + orow * p.ldr + nb : nullptr;
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (nb + r < n_out) c[r] = (f16_t)(val[r] + (rs ? (float)rs[r] : 0.f));
  }
}

// Weight-streaming form (M <= 64: decode steps, [SEG] rows, lm_head on the last rows), after gemm_nf4_kernel without the LUT: one
// workgroup per 16 * NT weight rows, KW waves splitting K into contiguous ranges of 64-byte blocks. Lane (fr, fh) holds weight row
// fr and activation row fr, bytes 16 fh .. 16 fh + 15 of a block: one 16-byte load each feeds v_mfma_i32_16x16x64_i8 directly
// (D[n = 4 fh + r][m = fr]). The KW int32 partial tiles are summed in LDS (exact).
template <int MT, int NT, bool SWIGLU, int KW>
__global__ __launch_bounds__(64 * KW) void gemm_i8_skinny_kernel(I8Args p) {
  static_assert(!SWIGLU || (NT % 2) == 0, "SwiGLU pairs a gate tile with an up tile");
  constexpr int U = quant_batch<MT>();
  __shared__ int red[KW][MT][64][4];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int fr = lane & 15, fh = lane >> 4;
  const int n0 = blockIdx.x * 16 * NT;
  const int kb = p.K >> 6;
  const int c_lo = (int)((long)wave * kb / KW), c_hi = (int)((long)(wave + 1) * kb / KW);
  const signed char* xrow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) xrow[mt] = p.CA + (long)min(mt * 16 + fr, p.M - 1) * p.ldca + 16 * fh;
  const signed char* wrow[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) wrow[t] = p.CB + (long)min(n0 + t * 16 + fr, p.N - 1) * p.K + 16 * fh;
  i32x4 acc[NT][MT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[t][mt] = i32x4{0, 0, 0, 0};
  uint4 wv[2][NT][U];
  uint4 xv[2][MT][U];
  auto load = [&](int set, int c) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int cc = min(c + u, c_hi - 1);     // tail: re-read, skipped at the MFMA
#pragma unroll
      for (int t = 0; t < NT; ++t) wv[set][t][u] = *reinterpret_cast<const uint4*>(wrow[t] + 64L * cc);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) xv[set][mt][u] = *reinterpret_cast<const uint4*>(xrow[mt] + 64L * cc);
    }
  };
  auto compute = [&](int set, int c) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (c + u < c_hi) {
#pragma unroll
        for (int t = 0; t < NT; ++t)
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) acc[t][mt] = mfma_i8(wv[set][t][u], xv[set][mt][u], acc[t][mt]);
      }
    }
  };
  if (c_lo < c_hi) {
    load(0, c_lo);
    for (int c = c_lo; c < c_hi; c += 2 * U) {
      if (c + U < c_hi) load(1, c + U);
      compute(0, c);
      if (c + U < c_hi) {
        if (c + 2 * U < c_hi) load(0, c + 2 * U);
        compute(1, c + U);
      }
    }
  }
  i32x4 o[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) *reinterpret_cast<i32x4*>(&red[wave][mt][lane][0]) = acc[t][mt];
    __syncthreads();
    if (wave < MT) {
      i32x4 sum = {0, 0, 0, 0};
#pragma unroll
      for (int w = 0; w < KW; ++w) sum += *reinterpret_cast<const i32x4*>(&red[w][wave][lane][0]);
      o[t] = sum;
    }
    if (t + 1 < NT) __syncthreads();
  }
  if (wave >= MT) return;
  const int m = wave * 16 + fr;
  if constexpr (SWIGLU) {
#pragma unroll
    for (int j = 0; j < NT / 2; ++j) i8_epilogue<true>(p, m, n0 + 32 * j, fh, o[2 * j], o[2 * j + 1]);
  } else {
#pragma unroll
    for (int t = 0; t < NT; ++t) i8_epilogue<false>(p, m, n0 + 16 * t, fh, o[t], o[t]);
  }
}

// Tiled form (prefill): workgroup = 128 weight rows x 64 activation rows, 4 waves of 32 x 64, 64-byte K steps staged through LDS
// (a 16-row fragment read is 1 KB contiguous: no bank conflicts), the next step's global loads in flight during the MFMAs.
constexpr int kTN = 128, kTM = 64;

template <bool SWIGLU>
__global__ __launch_bounds__(256) void gemm_i8_tiled_kernel(I8Args p) {
  __shared__ uint4 Ws[kTN * 4];
  __shared__ uint4 As[kTM * 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fr = lane & 15, fh = lane >> 4;
  const int m0 = blockIdx.x * kTM, n0 = blockIdx.y * kTN;
  const signed char* ws0 = p.CB + (long)min(n0 + (tid >> 2), p.N - 1) * p.K + 16 * (tid & 3);
  const signed char* ws1 = p.CB + (long)min(n0 + 64 + (tid >> 2), p.N - 1) * p.K + 16 * (tid & 3);
  const signed char* as = p.CA + (long)min(m0 + (tid >> 2), p.M - 1) * p.ldca + 16 * (tid & 3);
  const int kb = p.K >> 6;
  uint4 rw0 = *reinterpret_cast<const uint4*>(ws0), rw1 = *reinterpret_cast<const uint4*>(ws1);
  uint4 ra = *reinterpret_cast<const uint4*>(as);
  i32x4 acc[2][4];
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) acc[t][mt] = i32x4{0, 0, 0, 0};
  for (int c = 0; c < kb; ++c) {
    __syncthreads();
    Ws[tid] = rw0;
    Ws[tid + 256] = rw1;
    As[tid] = ra;
    __syncthreads();
    if (c + 1 < kb) {
      rw0 = *reinterpret_cast<const uint4*>(ws0 + 64L * (c + 1));
      rw1 = *reinterpret_cast<const uint4*>(ws1 + 64L * (c + 1));
      ra = *reinterpret_cast<const uint4*>(as + 64L * (c + 1));
    }
    uint4 w[2], x[4];
#pragma unroll
    for (int t = 0; t < 2; ++t) w[t] = Ws[(32 * wave + 16 * t + fr) * 4 + fh];
#pragma unroll
    for (int mt = 0; mt < 4; ++mt) x[mt] = As[(16 * mt + fr) * 4 + fh];
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
      for (int mt = 0; mt < 4; ++mt) acc[t][mt] = mfma_i8(w[t], x[mt], acc[t][mt]);
  }
  const int nt = n0 + 32 * wave;
#pragma unroll
  for (int mt = 0; mt < 4; ++mt) {
    const int m = m0 + 16 * mt + fr;
    if constexpr (SWIGLU) {
      i8_epilogue<true>(p, m, nt, fh, acc[0][mt], acc[1][mt]);
    } else {
      i8_epilogue<false>(p, m, nt, fh, acc[0][mt], acc[0][mt]);
      i8_epilogue<false>(p, m, nt + 16, fh, acc[1][mt], acc[1][mt]);
    }
  }
}

template <int MT>
void launch_i8_skinny(const I8Args& p, int swiglu, hipStream_t s) {
  const int nt = quant_raster_nt(p.N, MT, swiglu);
  const dim3 g = quant_grid(p.N, nt), b(64 * kQuantWaves);
  if (swiglu) hipLaunchKernelGGL((gemm_i8_skinny_kernel<MT, 2, true, kQuantWaves>), g, b, 0, s, p);
  else if (nt == 2) hipLaunchKernelGGL((gemm_i8_skinny_kernel<MT, 2, false, kQuantWaves>), g, b, 0, s, p);
  else hipLaunchKernelGGL((gemm_i8_skinny_kernel<MT, 1, false, kQuantWaves>), g, b, 0, s, p);
}

}  // namespace

extern "C" int haff_int8_quantize_weight_f16(const void* W, long ldw, int N, int K, const int* row_map, void* CB, float* SCB,
                                             void* stream) {
  if (N <= 0 || K <= 0 || (K & 63) || (ldw & 7) || ldw < K || !W || !CB || !SCB) return HAFF_ERR_BAD_ARG;
  if (!haff_aligned(W, 16) || !haff_aligned(CB, 16) || !haff_aligned(SCB, 4)) return HAFF_ERR_BAD_ARG;
  hipLaunchKernelGGL(i8_weight_kernel, dim3(N), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const f16_t*>(W),
                     ldw, K, row_map, reinterpret_cast<signed char*>(CB), SCB);
  return haff_check_launch();
}

extern "C" int haff_int8_quantize_act_f16(const void* A, long lda, int M, int K, float threshold, int seg_rows, const int* seg_valid,
                                          unsigned* masks, void* CA, long ldca, float* SCA, int* cols, int* ncols, void* stream) {
  if (M <= 0 || K <= 0 || (K & 63) || seg_rows <= 0 || (lda & 7) || lda < K || (ldca & 15) || ldca < K) return HAFF_ERR_BAD_ARG;
  if (!(threshold >= 0.f) || !A || !CA || !SCA || !cols || !ncols || (threshold > 0.f && !masks)) return HAFF_ERR_BAD_ARG;
  if (!haff_aligned(A, 16) || !haff_aligned(CA, 16) || !haff_aligned(SCA, 4) || !haff_aligned(masks, 4)) return HAFF_ERR_BAD_ARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int S = (M + seg_rows - 1) / seg_rows;
  const unsigned* mk = threshold > 0.f ? masks : nullptr;
  const f16_t* a = reinterpret_cast<const f16_t*>(A);
  if (seg_rows == 1 && (K >> 5) <= kI8RowMaxWords) {
    hipLaunchKernelGGL(i8_act_row_kernel, dim3(M), dim3(256), 0, s, a, lda, K, threshold, seg_valid, const_cast<unsigned*>(mk), SCA,
                       reinterpret_cast<signed char*>(CA), ldca, cols, ncols);
    return haff_check_launch();
  }
  hipLaunchKernelGGL(i8_act_scan_kernel, dim3(M), dim3(256), 0, s, a, lda, K, threshold, seg_rows, seg_valid, masks, SCA);
  hipLaunchKernelGGL(i8_act_codes_kernel, dim3(M), dim3(256), 0, s, a, lda, K, threshold, seg_rows, mk, SCA,
                     reinterpret_cast<signed char*>(CA), ldca);
  hipLaunchKernelGGL(i8_act_cols_kernel, dim3(S), dim3(256), 0, s, mk, K, cols, ncols);
  return haff_check_launch();
}

extern "C" int haff_gemm_int8_f16(const void* A, long lda, const void* CA, long ldca, const float* SCA, const void* CB, const float* SCB,
                                  const int* cols, const int* ncols, int seg_rows, void* C, long ldc, const float* bias, const void* resid,
                                  long ldr, const int* row_map, int M, int N, int K, int act, int out_f32, int swiglu, int form,
                                  void* stream) {
  if (M <= 0 || N <= 0 || K <= 0 || (K & 63) || seg_rows <= 0 || form < 0 || form > 2) return HAFF_ERR_BAD_ARG;
  if (!CA || !SCA || !CB || !SCB || !C || (ldca & 15) || ldca < K) return HAFF_ERR_BAD_ARG;
  if (!cols != !ncols || (ncols && (!A || lda < K))) return HAFF_ERR_BAD_ARG;
  if (!haff_aligned(CA, 16) || !haff_aligned(CB, 16) || !haff_aligned(SCA, 4) || !haff_aligned(SCB, 4)) return HAFF_ERR_BAD_ARG;
  if (swiglu && ((N & 31) || resid)) return HAFF_ERR_BAD_ARG;
  const int f = form ? form : (M <= 64 ? 1 : 2);
  if (f == 1 && M > 64) return HAFF_ERR_UNSUPPORTED;
  I8Args p{reinterpret_cast<const f16_t*>(A), lda, reinterpret_cast<const signed char*>(CA), ldca, SCA,
           reinterpret_cast<const signed char*>(CB), SCB, cols, ncols, seg_rows, C, ldc, bias, resid, ldr, row_map, M, N, K, act, out_f32};
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (f == 1) {
    HAFF_DISPATCH_MT(M, launch_i8_skinny<MT>(p, swiglu, s));
  } else {
    const dim3 g((M + kTM - 1) / kTM, (N + kTN - 1) / kTN);
    if (swiglu) hipLaunchKernelGGL(gemm_i8_tiled_kernel<true>, g, dim3(256), 0, s, p);
    else hipLaunchKernelGGL(gemm_i8_tiled_kernel<false>, g, dim3(256), 0, s, p);
  }
  return haff_check_launch();
}
