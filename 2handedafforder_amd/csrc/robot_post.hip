// Per-request post-processing of the reference's robot loop (2Haff/robot_demo.py:266-327) on the device, so that only the
// finished uint8 planes leave HBM.
//
//   haff_robot_heatmap : create_heatmap (:57-73) of each hand's fp32 logit plane: cv2.normalize(NORM_MINMAX, 0..255), np.uint8,
//                        applyColorMap(JET), GaussianBlur((5,5), 1). Restated from OpenCV 4.8 (cv2 is not a dependency here):
//                        scale = 255/(max-min) and shift = -min*scale in double (scale = 0 when max-min <= DBL_EPSILON),
//                        q = trunc(fmaf(x, (float)scale, (float)shift)); JET through a 256-entry RGB table (data, built by
//                        postprocess.jet_table); the bit-exact 8-bit blur: BORDER_REFLECT_101, separable fixed-point
//                        coefficients {14, 62, 104, 62, 14} / 256 (getGaussianKernelFixedPoint_ED of exp(-x^2/2), restated
//                        in tests/robot_ref.py), out = (sum c[dy] c[dx] p + 32768) >> 16 in integers only.
//                        Two launches: per-workgroup min/max partials (no atomics: every partial has its own slot), then
//                        one 64x16 output tile per workgroup that folds its plane's partials, quantises the 68x20 halo
//                        tile into LDS and runs the horizontal, then the vertical pass out of LDS.
//   haff_robot_mask    : `x > th` pasted at (left, top) into a zero plane of the padded size (PIL paste: negative margins
//                        crop), AND the lowest bit of the hand mask (cv2.bitwise_and of 0/1 with 0..255), times on_value.
// Both are HBM-bound byte work: one read of each 4-B logit, one write of each output byte.
#include "haff_common.h"

#include <float.h>

namespace {

constexpr int kParts = 256;                    // max min/max partials per plane (workspace: n * kParts * 2 floats)
constexpr int kTileW = 64, kTileH = 16;        // heatmap output tile per 256-thread workgroup (4 pixels per thread)
constexpr int kHaloW = kTileW + 4, kHaloH = kTileH + 4;

// min / max over a 256-thread workgroup; every thread gets the result
__device__ __forceinline__ void block_minmax(float& mn, float& mx, float* red /* [8] */) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) {
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { red[wave] = mn; red[4 + wave] = mx; }
  __syncthreads();
  mn = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
  mx = fmaxf(fmaxf(red[4], red[5]), fmaxf(red[6], red[7]));
}

// grid (parts, n): partials[plane][part] = (min, max) of the part's chunk (chunk a multiple of 4 elements).
__global__ __launch_bounds__(256) void robot_minmax_kernel(const float* logits, float* partials, long hw, long chunk,
                                                          int parts, int vec) {
  __shared__ float red[8];
  const float* p = logits + (long)blockIdx.y * hw;
  const long b = (long)blockIdx.x * chunk;
  const long e = b + chunk < hw ? b + chunk : hw;
  float mn = INFINITY, mx = -INFINITY;
  if (vec) {   // hw % 4 == 0 and a 16-B aligned base: every plane and every chunk starts 16-B aligned
    for (long i = b + 4 * (long)threadIdx.x; i < e; i += 4 * 256) {
      const float4 v = *reinterpret_cast<const float4*>(p + i);
      mn = fminf(mn, fminf(fminf(v.x, v.y), fminf(v.z, v.w)));
      mx = fmaxf(mx, fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)));
    }
  } else {
    for (long i = b + threadIdx.x; i < e; i += 256) {
      const float v = p[i];
      mn = fminf(mn, v);
      mx = fmaxf(mx, v);
    }
  }
  block_minmax(mn, mx, red);
  if (threadIdx.x == 0) {
    float* o = partials + ((long)blockIdx.y * parts + blockIdx.x) * 2;
    o[0] = mn;
    o[1] = mx;
  }
}

__device__ __forceinline__ unsigned char quantise(float x, float sc, float sh) {
  const float v = fmaf(x, sc, sh);
  int t = (int)v;                                   // np.uint8 of the float32 plane: truncation toward zero
  t = t < 0 ? 0 : (t > 255 ? 255 : t);
  return (unsigned char)t;
}

// grid (ceil(W/64), ceil(H/16), n); out u8 [n][H][W][3] in the RGB order the reference's PNG holds on disk
__global__ __launch_bounds__(256) void robot_heatmap_kernel(const float* logits, const float* partials,
                                                           const unsigned char* jet, unsigned char* out, int H, int W,
                                                           int parts, int vec) {
  __shared__ float red[8];
  __shared__ unsigned char lut[256 * 3];
  __shared__ unsigned char q[kHaloH][kHaloW];
  __shared__ unsigned short hsum[3][kHaloH][kTileW];
  const int tid = threadIdx.x;
  const int plane = blockIdx.z;
  const long hw = (long)H * W;
  const float* src = logits + plane * hw;

  for (int i = tid; i < 256 * 3; i += 256) lut[i] = jet[i];
  float mn = INFINITY, mx = -INFINITY;
  if (tid < parts) {
    const float* pp = partials + ((long)plane * parts + tid) * 2;
    mn = pp[0];
    mx = pp[1];
  }
  block_minmax(mn, mx, red);
  // cv::normalize(NORM_MINMAX, 0, 255): scale and shift in double, converted to float for the float32 convertTo
  const double d = (double)mx - (double)mn;
  const double scale = d > DBL_EPSILON ? 255.0 / d : 0.0;
  const double shift = -(double)mn * scale;
  const float sc = (float)scale, sh = (float)shift;

  // quantised halo tile: rows y0-2 .. y0+17, columns x0-2 .. x0+65, reflected; q[r][c] <- (y0-2+r, x0-2+c)
  const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  const bool full_row = vec && x0 + kTileW <= W;
  for (int i = tid; i < kHaloH * 16; i += 256) {      // interior columns x0 .. x0+63: 16 float4 per row
    const int r = i >> 4, c4 = i & 15;
    const long row = (long)reflect101(y0 - 2 + r, H) * W;
    if (full_row) {
      const float4 v = *reinterpret_cast<const float4*>(src + row + x0 + 4 * c4);
      q[r][2 + 4 * c4 + 0] = quantise(v.x, sc, sh);
      q[r][2 + 4 * c4 + 1] = quantise(v.y, sc, sh);
      q[r][2 + 4 * c4 + 2] = quantise(v.z, sc, sh);
      q[r][2 + 4 * c4 + 3] = quantise(v.w, sc, sh);
    } else {
#pragma unroll
      for (int k = 0; k < 4; ++k) q[r][2 + 4 * c4 + k] = quantise(src[row + reflect101(x0 + 4 * c4 + k, W)], sc, sh);
    }
  }
  if (tid < kHaloH * 4) {                               // two halo columns on each side
    const int r = tid >> 2, k = tid & 3;
    const int c = k < 2 ? k : kTileW + k;               // 0, 1, 66, 67
    q[r][c] = quantise(src[(long)reflect101(y0 - 2 + r, H) * W + reflect101(x0 - 2 + c, W)], sc, sh);
  }
  __syncthreads();

  // horizontal pass: hsum[ch][r][x] = sum_k c[k] * JET[q[r][x+k]][ch]  (<= 256 * 255: exact in u16)
  const int cf[5] = {14, 62, 104, 62, 14};
  for (int i = tid; i < kHaloH * kTileW; i += 256) {
    const int r = i / kTileW, x = i % kTileW;
    int s0 = 0, s1 = 0, s2 = 0;
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const unsigned char* e = lut + 3 * q[r][x + k];
      s0 += cf[k] * e[0];
      s1 += cf[k] * e[1];
      s2 += cf[k] * e[2];
    }
    hsum[0][r][x] = (unsigned short)s0;
    hsum[1][r][x] = (unsigned short)s1;
    hsum[2][r][x] = (unsigned short)s2;
  }
  __syncthreads();

  // vertical pass: 4 consecutive pixels of one row per thread, (sum + 2^15) >> 16
  const int r = tid >> 4, xc = (tid & 15) * 4;
  const int y = y0 + r, x = x0 + xc;
  if (y >= H || x >= W) return;
  unsigned char px[12];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
      int s = 32768;
#pragma unroll
      for (int k = 0; k < 5; ++k) s += cf[k] * hsum[ch][r + k][xc + j];
      px[3 * j + ch] = (unsigned char)(s >> 16);
    }
  unsigned char* o = out + (plane * hw + (long)y * W + x) * 3;
  if (x + 4 <= W && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
    unsigned* o4 = reinterpret_cast<unsigned*>(o);
#pragma unroll
    for (int w = 0; w < 3; ++w)
      o4[w] = px[4 * w] | (px[4 * w + 1] << 8) | (px[4 * w + 2] << 16) | ((unsigned)px[4 * w + 3] << 24);
  } else {
    const int nvalid = W - x < 4 ? W - x : 4;
    for (int j = 0; j < 3 * nvalid; ++j) o[j] = px[j];
  }
}

struct RobotMaskArgs {
  const float* logits;          // [H0][W0]
  const unsigned char* mask;    // [Ho][Wo] or nullptr
  unsigned char* out;           // [Ho][Wo]
  int H0, W0, Ho, Wo, left, top;
  float th;
  unsigned on;
};

// 4 consecutive output bytes per thread (one 4-B mask load, one 4-B store); the bytes of a last, partial quad one by one
__global__ __launch_bounds__(256) void robot_mask_kernel(RobotMaskArgs p) {
  const long total = (long)p.Ho * p.Wo;
  const long n4 = (total + 3) >> 2;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
    const long b = i << 2;
    const bool whole = b + 4 <= total;
    unsigned m = 0xffffffffu;
    if (p.mask) {
      if (whole) {
        m = *reinterpret_cast<const unsigned*>(p.mask + b);
      } else {
        m = 0;
        for (int k = 0; (long)k < total - b; ++k) m |= (unsigned)p.mask[b + k] << (8 * k);
      }
    }
    unsigned w = 0;
    int yy = (int)(b / p.Wo), xx = (int)(b % p.Wo);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int sy = yy - p.top, sx = xx - p.left;
      if (b + k < total && ((m >> (8 * k)) & 1u) && sy >= 0 && sy < p.H0 && sx >= 0 && sx < p.W0 &&
          p.logits[(long)sy * p.W0 + sx] > p.th)
        w |= p.on << (8 * k);
      if (++xx == p.Wo) { xx = 0; ++yy; }
    }
    if (whole) {
      *reinterpret_cast<unsigned*>(p.out + b) = w;
    } else {
      for (int k = 0; (long)k < total - b; ++k) p.out[b + k] = (unsigned char)(w >> (8 * k));
    }
  }
}

}  // namespace

extern "C" int haff_robot_heatmap(const float* logits, int n, int H, int W, const void* jet_rgb, float* workspace,
                                  long workspace_floats, void* out, void* stream) {
  if (!logits || !jet_rgb || !workspace || !out || n <= 0 || H <= 0 || W <= 0 || n > 65535) return HAFF_ERR_BAD_ARG;
  if (workspace_floats < (long)n * kParts * 2 || !haff_aligned(logits, 4)) return HAFF_ERR_BAD_ARG;
  const long hw = (long)H * W;
  if ((H + kTileH - 1) / kTileH > 65535) return HAFF_ERR_UNSUPPORTED;
  const int vec = (hw % 4 == 0) && haff_aligned(logits);
  long parts = (hw + 8191) / 8192;                      // >= 8192 elements (8 float4 per thread) per part
  if (parts > kParts) parts = kParts;
  const long chunk = ((hw + parts - 1) / parts + 3) & ~3L;
  parts = (hw + chunk - 1) / chunk;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(robot_minmax_kernel, dim3((unsigned)parts, (unsigned)n), dim3(256), 0, s, logits, workspace, hw, chunk,
                     (int)parts, vec);
  const dim3 grid((unsigned)((W + kTileW - 1) / kTileW), (unsigned)((H + kTileH - 1) / kTileH), (unsigned)n);
  hipLaunchKernelGGL(robot_heatmap_kernel, grid, dim3(256), 0, s, logits, workspace, (const unsigned char*)jet_rgb,
                     (unsigned char*)out, H, W, (int)parts, vec && (W % 4 == 0));
  return haff_check_launch();
}

extern "C" int haff_robot_mask(const float* logits, int H0, int W0, int left, int top, int right, int bottom, float th,
                               const void* mask, int mask_h, int mask_w, int on_value, void* out, void* stream) {
  if (!logits || !out || H0 <= 0 || W0 <= 0 || on_value < 0 || on_value > 255) return HAFF_ERR_BAD_ARG;
  const long Ho = (long)H0 + top + bottom, Wo = (long)W0 + left + right;
  if (Ho <= 0 || Wo <= 0 || Ho > INT32_MAX || Wo > INT32_MAX) return HAFF_ERR_BAD_ARG;
  if (mask && (mask_h != Ho || mask_w != Wo)) return HAFF_ERR_BAD_ARG;   // cv2.bitwise_and raises on a size mismatch
  if (!haff_aligned(out, 4) || !haff_aligned(mask, 4)) return HAFF_ERR_BAD_ARG;
  RobotMaskArgs p{logits, (const unsigned char*)mask, (unsigned char*)out, H0, W0, (int)Ho, (int)Wo, left, top, th,
                  (unsigned)on_value};
  long g = ((Ho * Wo + 3) / 4 + 255) / 256;
  if (g > 8192) g = 8192;
  hipLaunchKernelGGL(robot_mask_kernel, dim3((unsigned)g), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), p);
  return haff_check_launch();
}
