// Step 2 of the reference's benchmark workflow (ActAffordance/scripts/utils/gaussian.py: cv2.GaussianBlur(img, (7, 7), 0), then
// `blurred / 255.0 > threshold`, back to 0 / 255) moved in front of the thresholds, onto the fp32 logits.
//
//   haff_mask_quantile7 : out = the weighted upper quantile of the 49 BORDER_REFLECT_101 taps of every pixel, weights c[dy] c[dx]
//                         with c = {8, 28, 56, 72, 56, 28, 8} (OpenCV's built-in 7-tap table times 256; total 65536): the largest
//                         tap value v with weight{taps >= v} >= need.
//
// Why that is the smoothing: on a 0/255 plane p = 255 [logit > lt] the bit-exact 8-bit blur is (255 M + 32768) >> 16 with
// M = sum c[dy] c[dx] [logit(tap) > lt], and `blurred / 255.0 > tau` holds iff M >= need(tau) (need(0.5) = 32768, half the weight;
// postprocess.smooth_need). A weighted vote is monotone in the set of "on" taps, so for EVERY lt at once the smoothed mask is
// [quantile > lt]. The quantile is one of the inputs, no arithmetic touches it: each later `>` is the comparison the blurred file
// would give, bit for bit. NaN taps are off for every threshold (strict compares): they count as -inf, and a pixel whose weight of
// taps above -inf is below need gets -inf. No NaN is ever written.
//
// One 256-thread workgroup per 64x16 output tile (as robot_heatmap_kernel). The 70x22 halo tile goes to LDS as order-preserving
// uint32 keys; a thread takes 4 pixels of one column, 4 rows apart, so that a wave reads 64 consecutive keys (no bank conflict at
// any pitch) and stores 64 consecutive floats. Per pixel the 49 keys sit in registers and the answer is built bit by bit from the
// top: 32 steps, each the weight of {key >= candidate} from 49 compares counted into the 4x4 classes of equal weight (the kernel
// is symmetric), then 20 multiply-adds. VALU-bound: ~3500 lane operations per pixel against 8 B of HBM traffic.
#include "haff_common.h"

namespace {

constexpr int kTileW = 64, kTileH = 16;        // output tile per 256-thread workgroup (4 pixels per thread)
constexpr int kR = 3;                          // 7 taps per axis
constexpr int kHaloW = kTileW + 2 * kR, kHaloH = kTileH + 2 * kR;
constexpr unsigned kKeyNegInf = 0x007fffffu;   // key(-inf) = ~0xff800000

// float -> uint32 with a < b <=> key(a) < key(b); -0.0 joins +0.0 and NaN joins -inf
__device__ __forceinline__ unsigned to_key(float x) {
  if (x != x) return kKeyNegInf;
  const unsigned b = __float_as_uint(x + 0.0f);          // -0.0 + 0.0 = +0.0
  return (b & 0x80000000u) ? ~b : (b ^ 0x80000000u);
}
__device__ __forceinline__ float from_key(unsigned k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

// grid (ceil(W/64), ceil(H/16), min(n, 65535)); a workgroup walks the planes blockIdx.z, blockIdx.z + gridDim.z, ...
__global__ __launch_bounds__(256) void mask_quantile7_kernel(const float* logits, float* out, int n, int H, int W, int need,
                                                             int vec) {
  __shared__ unsigned key[kHaloH][kHaloW];
  const int tid = threadIdx.x;
  const long hw = (long)H * W;
  const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  const bool full_row = vec && x0 + kTileW <= W;
  const int col = tid & 63, row0 = tid >> 6;
  const int wc[4] = {8, 28, 56, 72};

  for (int plane = blockIdx.z; plane < n; plane += gridDim.z) {
    const float* src = logits + plane * hw;
    // key[r][c] <- (y0 - 3 + r, x0 - 3 + c), reflected
    for (int i = tid; i < kHaloH * 16; i += 256) {        // interior columns x0 .. x0+63: 16 float4 per row
      const int r = i >> 4, c4 = i & 15;
      const long row = (long)reflect101(y0 - kR + r, H) * W;
      if (full_row) {
        const float4 v = *reinterpret_cast<const float4*>(src + row + x0 + 4 * c4);
        key[r][kR + 4 * c4 + 0] = to_key(v.x);
        key[r][kR + 4 * c4 + 1] = to_key(v.y);
        key[r][kR + 4 * c4 + 2] = to_key(v.z);
        key[r][kR + 4 * c4 + 3] = to_key(v.w);
      } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) key[r][kR + 4 * c4 + k] = to_key(src[row + reflect101(x0 + 4 * c4 + k, W)]);
      }
    }
    if (tid < kHaloH * 2 * kR) {                          // three halo columns on each side
      const int r = tid / (2 * kR), k = tid % (2 * kR);
      const int c = k < kR ? k : kTileW + k;              // 0, 1, 2, 67, 68, 69
      key[r][c] = to_key(src[(long)reflect101(y0 - kR + r, H) * W + reflect101(x0 - kR + c, W)]);
    }
    __syncthreads();

    const int x = x0 + col;
    if (x < W) {
#pragma unroll 1
      for (int j = 0; j < 4; ++j) {
        const int r = row0 + 4 * j;
        if (y0 + r >= H) break;
        unsigned t[49];
#pragma unroll
        for (int dy = 0; dy < 7; ++dy)
#pragma unroll
          for (int dx = 0; dx < 7; ++dx) t[dy * 7 + dx] = key[r + dy][col + dx];
        unsigned ans = 0;                                 // weight{key >= 0} = 65536 >= need
#pragma unroll 1
        for (int bit = 31; bit >= 0; --bit) {
          const unsigned cand = ans | (1u << bit);
          int cnt[4][4] = {};
#pragma unroll
          for (int dy = 0; dy < 7; ++dy)
#pragma unroll
            for (int dx = 0; dx < 7; ++dx) cnt[dy < 4 ? dy : 6 - dy][dx < 4 ? dx : 6 - dx] += t[dy * 7 + dx] >= cand ? 1 : 0;
          int mass = 0;
#pragma unroll
          for (int a = 0; a < 4; ++a)
            mass += wc[a] * (wc[0] * cnt[a][0] + wc[1] * cnt[a][1] + wc[2] * cnt[a][2] + wc[3] * cnt[a][3]);
          if (mass >= need) ans = cand;
        }
        out[plane * hw + (long)(y0 + r) * W + x] = from_key(ans);
      }
    }
    __syncthreads();                                      // the next plane overwrites the tile
  }
}

}  // namespace

extern "C" int haff_mask_quantile7(const float* logits, int n, int H, int W, int need, float* out, void* stream) {
  if (!logits || !out || logits == out || n < 1 || H < 1 || W < 1 || need < 1 || need > 65536) return HAFF_ERR_BAD_ARG;
  if (!haff_aligned(logits, 4) || !haff_aligned(out, 4)) return HAFF_ERR_BAD_ARG;
  if (H > 4096 || W > 4096) return HAFF_ERR_UNSUPPORTED;
  const int vec = (W % 4 == 0) && haff_aligned(logits);
  const dim3 grid((unsigned)((W + kTileW - 1) / kTileW), (unsigned)((H + kTileH - 1) / kTileH), (unsigned)(n < 65535 ? n : 65535));
  hipLaunchKernelGGL(mask_quantile7_kernel, grid, dim3(256), 0, reinterpret_cast<hipStream_t>(stream), logits, out, n, H, W, need,
                     vec);
  return haff_check_launch();
}
