// Building 2HANDS records from hand and object masks (2HANDS/scripts/affordance_extraction_preparation.py:256-304 as cvlite restates
// it): the mask arithmetic in front of the contour walk.
//
//   haff_affordance_extract : one launch processes a batch of planes of any mix of shapes. Per item (ExtractItem, a 64-byte descriptor
//                             the host uploads): a u8 plane `in` [H][W], an optional u8 hand mask [Hh][Wh] read through two int32
//                             gather tables col[W] / row[H] (the nearest resize of the hand padded to a square, built on the host in
//                             double as OpenCV does; -1 = the padding), an optional u8 output [H][W].
//
//   a(y, x)   = in(y, x) & hand[row[y]][col[x]]  (bitwise, as cv2.bitwise_and: 1 & 2 is 0; 0 where either index is -1), or in(y, x)
//               without a hand.
//   out(y, x) = 255 if any a(y', x') != 0 with x' in [x - k/2, x + k - 1 - k/2], y' likewise, inside the image, else 0:
//               cv2.dilate with a k x k rectangle, default anchor (k/2, k/2), the default border (taps outside the image stay out of
//               the maximum), then recolor_masks_white. For even k the window reaches one pixel further to the LEFT of a set pixel
//               than to its right: a pixel at column 5 turns on 4..7 for k = 4.
//   stats     i64 [n][8] = {non-zero pixels of a, non-zero pixels of out, sum of a, min row, max row, min column, max column of out's
//               on pixels, flags}; an empty plane leaves min = H (rows) / W (columns) and max = -1.
//
// Grid (tiles of the largest item, items), 256 threads, one workgroup per 16 x 64 output tile. The four waves read the tile plus its
// k - 1 halo row by row (128 columns from x0 - 32, the lanes outside [x0 - k/2, x0 + 63 + k - 1 - k/2] stay idle), a ballot turns
// `a != 0` into two 64-bit words per row in LDS. One thread per row ORs the k shifted windows (horizontal pass), one thread per
// output row ORs k rows (vertical pass), then every thread expands four bits into one 4-byte store (bytes where the address or the
// row's end does not allow it). Statistics: popcounts and first / last set bits of the words, reduced in LDS, then one integer
// atomic per counter and workgroup. Integer sums, minima and maxima do not depend on arrival order: repeat runs are bitwise equal.
#include "haff_common.h"

namespace {

constexpr int kMaxSide = 4096;
constexpr int kMaxK = 31;
constexpr int kTileH = 16, kTileW = 64;
constexpr int kMaxRows = kTileH + kMaxK - 1;   // tile plus halo
constexpr int kLead = 32;                      // columns in front of the tile in a row's 128-bit window

struct ExtractItem {                // == haff_extract_item (include/haff_hip.h)
  const unsigned char* in;          // [H][W]
  const unsigned char* hand;        // [Hh][Wh] or null
  const int* col;                   // [W] with a hand
  const int* row;                   // [H] with a hand
  unsigned char* out;               // [H][W] or null (statistics only)
  int H, W, Hh, Wh;
  int pad[2];
};
static_assert(sizeof(ExtractItem) == 64, "descriptor layout");
HAFF_SAME_SIZE(ExtractItem, haff_extract_item);
HAFF_SAME_FIELD(ExtractItem, in, haff_extract_item, in);
HAFF_SAME_FIELD(ExtractItem, hand, haff_extract_item, hand);
HAFF_SAME_FIELD(ExtractItem, col, haff_extract_item, col);
HAFF_SAME_FIELD(ExtractItem, row, haff_extract_item, row);
HAFF_SAME_FIELD(ExtractItem, out, haff_extract_item, out);
HAFF_SAME_FIELD(ExtractItem, H, haff_extract_item, H);
HAFF_SAME_FIELD(ExtractItem, W, haff_extract_item, W);
HAFF_SAME_FIELD(ExtractItem, Hh, haff_extract_item, Hh);
HAFF_SAME_FIELD(ExtractItem, Wh, haff_extract_item, Wh);
HAFF_SAME_FIELD(ExtractItem, pad, haff_extract_item, pad);

typedef unsigned long long u64;

__global__ void extract_init_kernel(const ExtractItem* items, int n, long long* stats) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const ExtractItem it = items[i];
  long long* s = stats + 8L * i;
  s[0] = 0; s[1] = 0; s[2] = 0;
  s[3] = it.H; s[4] = -1;
  s[5] = it.W; s[6] = -1;
  s[7] = it.hand ? 1 : 0;
}

// bits b .. b + 63 of the 128-bit window {lo, hi}, 0 < b < 64
__device__ __forceinline__ u64 window64(u64 lo, u64 hi, int b) { return (lo >> b) | (hi << (64 - b)); }

__global__ __launch_bounds__(256) void affordance_extract_kernel(const ExtractItem* items, int k, long long* stats) {
  __shared__ u64 bits[kMaxRows][2];
  __shared__ u64 hor[kMaxRows];
  __shared__ u64 res[kTileH];
  __shared__ unsigned s_nz_a, s_nz_out, s_sum, s_grey;
  __shared__ int s_min_r, s_max_r, s_min_c, s_max_c;

  const ExtractItem it = items[blockIdx.y];
  const int tiles_x = (it.W + kTileW - 1) / kTileW, tiles_y = (it.H + kTileH - 1) / kTileH;
  if ((int)blockIdx.x >= tiles_x * tiles_y) return;   // a smaller item of the batch: the whole workgroup leaves, before any barrier
  const int x0 = ((int)blockIdx.x % tiles_x) * kTileW, y0 = ((int)blockIdx.x / tiles_x) * kTileH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int L = k / 2, R = k - 1 - L;                 // the window's reach to smaller and to larger indices
  const int n_rows = kTileH + k - 1;

  if (tid == 0) {
    s_nz_a = 0; s_nz_out = 0; s_sum = 0; s_grey = 0;
    s_min_r = it.H; s_max_r = -1; s_min_c = it.W; s_max_c = -1;
  }

  // every lane of a wave runs every iteration (the ballots see the full wave); a lane outside the image or the halo contributes 0
  unsigned sum = 0, grey = 0;
  for (int i = wave; i < n_rows; i += 4) {
    const int y = y0 - L + i;
    const bool row_in = y >= 0 && y < it.H;
    const int hr = (row_in && it.hand) ? it.row[y] : -1;
    const bool own_row = i >= L && i < L + kTileH;
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      const int x = x0 - kLead + half * 64 + lane;
      unsigned v = 0;
      if (row_in && x >= 0 && x < it.W && x >= x0 - L && x <= x0 + kTileW - 1 + R) {
        v = it.in[(long)y * it.W + x];
        if (it.hand && v) {
          const int hc = it.col[x];
          unsigned h = 0;
          if ((unsigned)hr < (unsigned)it.Hh && (unsigned)hc < (unsigned)it.Wh) h = it.hand[(long)hr * it.Wh + hc];
          v &= h;
        }
        if (own_row && x >= x0 && x < x0 + kTileW) {
          sum += v;
          grey |= (v != 0 && v != 255) ? 1u : 0u;
        }
      }
      const u64 b = __ballot(v != 0);
      if (lane == 0) bits[i][half] = b;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    sum += __shfl_xor(sum, o, 64);
    grey |= __shfl_xor(grey, o, 64);
  }
  __syncthreads();
  if (lane == 0) {
    if (sum) atomicAdd(&s_sum, sum);
    if (grey) atomicOr(&s_grey, grey);
  }

  // horizontal pass: output bit j of a row sits at window position kLead + j and is on when a bit at kLead + j + s is, s in [-L, R]
  if (tid < n_rows) {
    const u64 lo = bits[tid][0], hi = bits[tid][1];
    u64 h = 0;
    for (int s = -L; s <= R; ++s) h |= window64(lo, hi, kLead + s);
    hor[tid] = h;
    if (tid >= L && tid < L + kTileH) {
      const unsigned c = (unsigned)__popcll(window64(lo, hi, kLead));
      if (c) atomicAdd(&s_nz_a, c);
    }
  }
  __syncthreads();

  // vertical pass: output row y0 + t ORs the halo rows t .. t + k - 1
  if (tid < kTileH) {
    const int y = y0 + tid;
    u64 o = 0;
    if (y < it.H) {
      for (int i = tid; i < tid + k; ++i) o |= hor[i];
      const int live = it.W - x0;                     // columns of this tile inside the image, >= 1
      if (live < kTileW) o &= (1ull << live) - 1ull;
    }
    res[tid] = o;
    if (o) {
      atomicAdd(&s_nz_out, (unsigned)__popcll(o));
      atomicMin(&s_min_r, y);
      atomicMax(&s_max_r, y);
      atomicMin(&s_min_c, x0 + __ffsll((long long)o) - 1);
      atomicMax(&s_max_c, x0 + 63 - __clzll((long long)o));
    }
  }
  __syncthreads();

  if (it.out) {
    const int y = y0 + (tid >> 4), x = x0 + (tid & 15) * 4;
    if (y < it.H && x < it.W) {
      const unsigned nib = (unsigned)(res[tid >> 4] >> ((tid & 15) * 4)) & 15u;
      const unsigned w = ((nib & 1u) ? 0xffu : 0u) | ((nib & 2u) ? 0xff00u : 0u) | ((nib & 4u) ? 0xff0000u : 0u) |
                         ((nib & 8u) ? 0xff000000u : 0u);
      unsigned char* o = it.out + (long)y * it.W + x;
      if (x + 4 <= it.W && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
        *reinterpret_cast<unsigned*>(o) = w;
      } else {
        for (int j = 0; j < 4 && x + j < it.W; ++j) o[j] = (unsigned char)(w >> (8 * j));
      }
    }
  }

  if (tid == 0) {
    long long* s = stats + 8L * blockIdx.y;
    if (s_nz_a) atomicAdd(reinterpret_cast<u64*>(s + 0), (u64)s_nz_a);
    if (s_sum) atomicAdd(reinterpret_cast<u64*>(s + 2), (u64)s_sum);
    if (s_grey) atomicOr(reinterpret_cast<u64*>(s + 7), 2ull);
    if (s_nz_out) {
      atomicAdd(reinterpret_cast<u64*>(s + 1), (u64)s_nz_out);
      atomicMin(s + 3, (long long)s_min_r);
      atomicMax(s + 4, (long long)s_max_r);
      atomicMin(s + 5, (long long)s_min_c);
      atomicMax(s + 6, (long long)s_max_c);
    }
  }
}

}  // namespace

extern "C" int haff_affordance_extract(const void* items_host, const void* items_dev, int n_items, int k, void* stats, void* stream) {
  if (!items_host || !items_dev || !stats || n_items <= 0 || n_items > 65535) return HAFF_ERR_BAD_ARG;
  if (!haff_aligned(items_host, 8) || !haff_aligned(items_dev, 8) || !haff_aligned(stats, 8)) return HAFF_ERR_BAD_ARG;
  if (k < 1 || k > kMaxK) return HAFF_ERR_UNSUPPORTED;
  const ExtractItem* items = static_cast<const ExtractItem*>(items_host);
  long tiles = 1;
  for (int i = 0; i < n_items; ++i) {
    const ExtractItem& it = items[i];
    if (!it.in || it.H <= 0 || it.W <= 0 || it.in == it.out) return HAFF_ERR_BAD_ARG;
    if (it.hand) {
      if (!it.col || !it.row || it.Hh <= 0 || it.Wh <= 0) return HAFF_ERR_BAD_ARG;
      if (!haff_aligned(it.col, 4) || !haff_aligned(it.row, 4)) return HAFF_ERR_BAD_ARG;
      if (it.Hh > kMaxSide || it.Wh > kMaxSide) return HAFF_ERR_UNSUPPORTED;
    }
    if (it.H > kMaxSide || it.W > kMaxSide) return HAFF_ERR_UNSUPPORTED;
    const long t = (long)((it.W + kTileW - 1) / kTileW) * ((it.H + kTileH - 1) / kTileH);
    tiles = t > tiles ? t : tiles;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(extract_init_kernel, dim3((unsigned)((n_items + 255) / 256)), dim3(256), 0, s,
                     static_cast<const ExtractItem*>(items_dev), n_items, (long long*)stats);
  hipLaunchKernelGGL(affordance_extract_kernel, dim3((unsigned)tiles, (unsigned)n_items), dim3(256), 0, s,
                     static_cast<const ExtractItem*>(items_dev), k, (long long*)stats);
  return haff_check_launch();
}
