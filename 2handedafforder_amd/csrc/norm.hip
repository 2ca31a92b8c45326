// Row normalisation kernels (HBM-bound): one 64-lane wave per row, 16-byte vector loads, fp32 statistics.
//
//   haff_layernorm : nn.LayerNorm over the last dim, biased variance, y = (x-mean)/sqrt(var+eps)*w+b
//       SAM encoder norm1/norm2 eps 1e-6 (build_sam.py:77, image_encoder.py:160,170,179,191)
//       LayerNorm2d of the neck / upscaler on channels-last data (common.py:31-43)
//       SAM decoder norms eps 1e-5 (transformer.py:60,134-144); CLIP pre_layrnorm / layer_norm1/2 eps 1e-5
//     with an optional GATHER map: out row i reads in row in_map[i]; in_map[i] < 0 writes zeros. This fuses
//     window_partition's zero padding, which the reference applies AFTER norm1 (image_encoder.py:179-183,276-288).
//   haff_rmsnorm  : Llama RMSNorm, fp32 variance (transformers LlamaRMSNorm; input/post-attention/final norm)
#include "haff_common.h"

namespace {

template <typename T, int NCH, bool RMS, typename TO = T>
__global__ __launch_bounds__(256) void norm_rows_kernel(const T* x, long ldx, TO* y, long ldy, const float* w,
                                                       const float* bvec, const int* in_map, int rows, int C,
                                                       float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  long src = row;
  if (in_map) {
    const int mrow = in_map[row];
    if (mrow < 0) {
      const float z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
      for (int i = 0; i < NCH; ++i) {
        const int c = (lane + 64 * i) * 8;
        if (c < C) store8(y + (long)row * ldy + c, z);
      }
      return;
    }
    src = mrow;
  }
  float v[NCH][8];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = (lane + 64 * i) * 8;
    if (c < C) {
      load8(x + src * ldx + c, v[i]);
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += RMS ? v[i][j] * v[i][j] : v[i][j];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[i][j] = 0.f;
    }
  }
  sum = wave_sum(sum);
  float mean = 0.f, rstd;
  if (RMS) {
    rstd = 1.0f / sqrtf(sum / (float)C + eps);
  } else {
    mean = sum / (float)C;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = (lane + 64 * i) * 8;
      if (c < C) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float dlt = v[i][j] - mean;
          sq += dlt * dlt;
        }
      }
    }
    sq = wave_sum(sq);
    rstd = 1.0f / sqrtf(sq / (float)C + eps);
  }
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = (lane + 64 * i) * 8;
    if (c < C) {
      float wv[8], o[8];
      load8(w + c, wv);
      if (RMS) {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = v[i][j] * rstd * wv[j];
      } else {
        float bb[8];
        load8(bvec + c, bb);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (v[i][j] - mean) * rstd * wv[j] + bb[j];
      }
      store8(y + (long)row * ldy + c, o);
    }
  }
}

// Few wide rows (KV-cached decode steps: 1..64 rows of 4096 / 5120): one WORKGROUP per row — 256 lanes x 16-B loads cover
// 4 KiB per pass, the two statistics meet in LDS. One wave per row left 1..16 workgroups on the chip with 8-10 dependent
// loads each: 14 us per call at 64 x 4096, 7.8 us at 1 x 4096 — two calls per layer of every decode step.
template <typename T, int NCH, bool RMS, typename TO = T>
__global__ __launch_bounds__(256) void norm_row_wg_kernel(const T* x, long ldx, TO* y, long ldy, const float* w,
                                                         const float* bvec, int C, float eps) {
  __shared__ float red[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const long row = blockIdx.x;
  float v[NCH][8];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = (tid + 256 * i) * 8;
    if (c < C) {
      load8(x + row * ldx + c, v[i]);
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += RMS ? v[i][j] * v[i][j] : v[i][j];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[i][j] = 0.f;
    }
  }
  sum = wave_sum(sum);
  if (lane == 0) red[0][wave] = sum;
  __syncthreads();
  sum = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
  float mean = 0.f, rstd;
  if (RMS) {
    rstd = 1.0f / sqrtf(sum / (float)C + eps);
  } else {
    mean = sum / (float)C;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = (tid + 256 * i) * 8;
      if (c < C) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float dlt = v[i][j] - mean;
          sq += dlt * dlt;
        }
      }
    }
    sq = wave_sum(sq);
    if (lane == 0) red[1][wave] = sq;
    __syncthreads();
    sq = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
    rstd = 1.0f / sqrtf(sq / (float)C + eps);
  }
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = (tid + 256 * i) * 8;
    if (c < C) {
      float wv[8], o[8];
      load8(w + c, wv);
      if (RMS) {
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = v[i][j] * rstd * wv[j];
      } else {
        float bb[8];
        load8(bvec + c, bb);
#pragma unroll
        for (int j = 0; j < 8; ++j) o[j] = (v[i][j] - mean) * rstd * wv[j] + bb[j];
      }
      store8(y + row * ldy + c, o);
    }
  }
}

template <typename T, bool RMS, typename TO = T>
int launch_norm(const void* x, long ldx, void* y, long ldy, const float* w, const float* b, const int* in_map,
                int rows, int C, float eps, hipStream_t s) {
  if (!in_map && rows <= 256 && C >= 2048 && C <= 3 * 2048) {
    const T* xp = reinterpret_cast<const T*>(x);
    TO* yp = reinterpret_cast<TO*>(y);
    if (C <= 2048) hipLaunchKernelGGL((norm_row_wg_kernel<T, 1, RMS, TO>), dim3(rows), dim3(256), 0, s, xp, ldx, yp, ldy, w, b, C, eps);
    else if (C <= 4096) hipLaunchKernelGGL((norm_row_wg_kernel<T, 2, RMS, TO>), dim3(rows), dim3(256), 0, s, xp, ldx, yp, ldy, w, b, C, eps);
    else hipLaunchKernelGGL((norm_row_wg_kernel<T, 3, RMS, TO>), dim3(rows), dim3(256), 0, s, xp, ldx, yp, ldy, w, b, C, eps);
    return haff_check_launch();
  }
  const int nch = (C + 511) / 512;
  dim3 grid((rows + 3) / 4), block(256);
  const T* xp = reinterpret_cast<const T*>(x);
  TO* yp = reinterpret_cast<TO*>(y);
#define HAFF_NORM_CASE(N)                                                                                   \
  if (nch <= N) {                                                                                           \
    hipLaunchKernelGGL((norm_rows_kernel<T, N, RMS, TO>), grid, block, 0, s, xp, ldx, yp, ldy, w, b, in_map, rows, C, eps); \
    return haff_check_launch();                                                                             \
  }
  HAFF_NORM_CASE(1)
  HAFF_NORM_CASE(2)
  HAFF_NORM_CASE(3)
  HAFF_NORM_CASE(4)
  HAFF_NORM_CASE(8)
  HAFF_NORM_CASE(10)
  HAFF_NORM_CASE(16)
#undef HAFF_NORM_CASE
  return HAFF_ERR_UNSUPPORTED;
}

// Row statistics only: stats[row] = {mean, rstd} (RMS: {0, rsqrt(mean(x^2) + eps)}). Half the HBM traffic of the norm
// itself (no normalised copy is written); the consumer GEMM applies them in its epilogue (haff_gemm_bf16_ln).
template <typename T, int NCH, bool RMS>
__global__ __launch_bounds__(256) void row_stats_kernel(const T* x, long ldx, float* stats, int rows, int C, float eps) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  float v[NCH][8];
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NCH; ++i) {
    const int c = (lane + 64 * i) * 8;
    if (c < C) {
      load8(x + (long)row * ldx + c, v[i]);
#pragma unroll
      for (int j = 0; j < 8; ++j) sum += RMS ? v[i][j] * v[i][j] : v[i][j];
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) v[i][j] = 0.f;
    }
  }
  sum = wave_sum(sum);
  float mean = 0.f, rstd;
  if (RMS) {
    rstd = 1.0f / sqrtf(sum / (float)C + eps);
  } else {
    mean = sum / (float)C;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < NCH; ++i) {
      const int c = (lane + 64 * i) * 8;
      if (c < C) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float dlt = v[i][j] - mean;
          sq += dlt * dlt;
        }
      }
    }
    sq = wave_sum(sq);
    rstd = 1.0f / sqrtf(sq / (float)C + eps);
  }
  if (lane == 0) *reinterpret_cast<float2*>(stats + 2 * (long)row) = make_float2(mean, rstd);
}

template <typename T, bool RMS>
int launch_stats(const void* x, long ldx, float* stats, int rows, int C, float eps, hipStream_t s) {
  const int nch = (C + 511) / 512;
  dim3 grid((rows + 3) / 4), block(256);
  const T* xp = reinterpret_cast<const T*>(x);
#define HAFF_STATS_CASE(N)                                                                             \
  if (nch <= N) {                                                                                      \
    hipLaunchKernelGGL((row_stats_kernel<T, N, RMS>), grid, block, 0, s, xp, ldx, stats, rows, C, eps); \
    return haff_check_launch();                                                                        \
  }
  HAFF_STATS_CASE(1)
  HAFF_STATS_CASE(2)
  HAFF_STATS_CASE(3)
  HAFF_STATS_CASE(4)
  HAFF_STATS_CASE(8)
  HAFF_STATS_CASE(10)
  HAFF_STATS_CASE(16)
#undef HAFF_STATS_CASE
  return HAFF_ERR_UNSUPPORTED;
}

// the norms' four-way type choice: code 2 is theirs alone, the other codes are the common three
template <bool RMS>
int launch_norm_dtype(const void* x, long ldx, void* y, long ldy, const float* w, const float* b, const int* in_map, int rows, int C,
                      float eps, int dtype, void* stream) {
  if (dtype == 2) return launch_norm<float, RMS, bf16_t>(x, ldx, y, ldy, w, b, in_map, rows, C, eps, haff_stream(stream));
  HAFF_DISPATCH(dtype, return launch_norm<T, RMS>(x, ldx, y, ldy, w, b, in_map, rows, C, eps, haff_stream(stream)));
  return HAFF_ERR_BAD_ARG;   // not reached: every case above returns
}

}  // namespace

// dtype: 0 = bf16, 1 = f32 (x and y), 2 = f32 x -> bf16 y (an fp32 residual stream feeding a bf16 product: one rounding, of the
// NORMALISED row), 3 = f16 (x and y). w, b fp32 [C]. C % 8 == 0, C <= 8192, ldx/ldy % 8 == 0.
extern "C" int haff_layernorm(const void* x, long ldx, void* y, long ldy, const float* w, const float* b,
                              const int* in_map, int rows, int C, float eps, int dtype, void* stream) {
  if (rows <= 0 || C <= 0 || (C & 7) || (ldx & 7) || (ldy & 7) || !w || !b || dtype < 0 || dtype > 3) return HAFF_ERR_BAD_ARG;
  return launch_norm_dtype<false>(x, ldx, y, ldy, w, b, in_map, rows, C, eps, dtype, stream);
}

extern "C" int haff_rmsnorm(const void* x, long ldx, void* y, long ldy, const float* w, int rows, int C,
                            float eps, int dtype, void* stream) {
  if (rows <= 0 || C <= 0 || (C & 7) || (ldx & 7) || (ldy & 7) || !w || dtype < 0 || dtype > 3) return HAFF_ERR_BAD_ARG;
  return launch_norm_dtype<true>(x, ldx, y, ldy, w, nullptr, nullptr, rows, C, eps, dtype, stream);
}

// {mean, rstd} from the per-wave partial sums haff_gemm_bf16_rowstats left: partials f32 [rows][slots][2] = {sum, sum of squares}
// over 64 columns each, added in slot order (deterministic); C = the row length the sums cover.
namespace {
__global__ __launch_bounds__(256) void row_stats_finalize_kernel(const float* part, float* stats, int rows, int slots, int C,
                                                                 float eps) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= rows) return;
  const float2* p = reinterpret_cast<const float2*>(part) + (long)r * slots;
  // E[x^2] - mean^2 cancels when |mean| >> std: the slot sums arrive as fp32 (each the sum of 64 fp32 products: ~5e-7
  // relative), so the variance carries ~5e-7 * (mean / std)^2 whatever is done here (the two-pass haff_row_stats has no such
  // term). Adding the slots, dividing by C and forming the difference in double contributes 2^-53 * (mean / std)^2 and no more —
  // but only with the division in double too: multiplying by an fp32 1 / C scales E[x^2] and mean^2 by (1 + e) and (1 + e)^2
  // (e = 1.5e-8 at C = 1280) and leaves -e * mean^2 in the variance, 1.5e-2 of it at mean / std = 1000.
  // tests/test_ops_gpu.py::test_linear_rowstats_with_a_large_row_mean holds the bound on a GEMM's partials at mean / std = 30 and
  // 100, tests/test_norm_ingest_kernels_gpu.py::test_row_stats_finalize_exact_partials on exact partials up to 1000.
  double s1 = 0.0, s2 = 0.0;
  for (int i = 0; i < slots; ++i) {
    const float2 v = p[i];
    s1 += (double)v.x;
    s2 += (double)v.y;
  }
  const double mean = s1 / (double)C;
  const double var = fmax(s2 / (double)C - mean * mean, 0.0);
  reinterpret_cast<float2*>(stats)[r] = float2{(float)mean, (float)(1.0 / sqrt(var + (double)eps))};
}
}  // namespace

extern "C" int haff_row_stats_finalize(const float* partials, float* stats, int rows, int slots, int C, float eps, void* stream) {
  if (rows <= 0 || slots <= 0 || C <= 0 || !partials || !stats) return HAFF_ERR_BAD_ARG;
  hipLaunchKernelGGL(row_stats_finalize_kernel, dim3((rows + 255) / 256), dim3(256), 0, haff_stream(stream),
                     partials, stats, rows, slots, C, eps);
  return haff_check_launch();
}

// stats[rows][2] = {mean, rstd} of each row (rms != 0: {0, rsqrt(mean(x^2) + eps)} — LlamaRMSNorm). dtype: 0 = bf16,
// 1 = f32, 3 = f16, any other code is refused. For haff_gemm_bf16_ln, which applies the normalisation inside the consumer product.
extern "C" int haff_row_stats(const void* x, long ldx, float* stats, int rows, int C, float eps, int rms, int dtype,
                              void* stream) {
  if (rows <= 0 || C <= 0 || (C & 7) || (ldx & 7) || !stats) return HAFF_ERR_BAD_ARG;
  HAFF_DISPATCH(dtype, HAFF_DISPATCH_BOOL(rms, RMS, return launch_stats<T, RMS>(x, ldx, stats, rows, C, eps, haff_stream(stream))));
  return HAFF_ERR_BAD_ARG;   // not reached: every case above returns
}
