// The object-crop augmentation on the device (train_ds.py --aug_crop with --device_ingest): the middle one of the three offline
// augmentations of the 2HANDS training set (2HANDS/scripts/data_augmentation/process_cropped_sequences.py, crop_and_pad) per sample,
// byte for byte what Pillow gives. For a sample of size (H, W) with the box (x0, y0, cw, ch) pasted at (px, py) on a black square of
// side S = max(cw, ch):
//
//   Q[sy][sx] = src[y0 + sy - py][x0 + sx - px] inside the pasted window, 0 elsewhere        (Image.crop, Image.new, paste)
//   out       = Q.resize((W, H), BICUBIC): the horizontal pass S -> W, a uint8 intermediate [S][W], the vertical pass S -> H,
//               each  clip8((2^21 + sum of in * k) >> 22)  with Pillow's 22-bit coefficients (preprocess.pil_resample_tables, built
//               on the host: Pillow normalises them in double, so they are never recomputed here).
//
// haff_crop_resample_u8 : ONE kernel, a block per 16 x 64 output tile of one sample. The block resamples the source rows its 16
//                         output rows reach (at most 96: 16 rows at a 4-fold down-scale and 17 taps) horizontally for its 64 columns
//                         into LDS, then the vertical pass reads that uint8 intermediate from LDS. Q and the intermediate never exist
//                         in HBM: the source window is read once per tile column (neighbouring tiles share the taps' halo through
//                         L2) and the output is written once.
//   mirror (flag bit 0)  : src is read with every row reversed, so the flip and the crop cost one pass and the box is the MIRRORED
//                          planes' box (its x1 is exclusive while max_x is inclusive: the crop of the mirror is not the mirror of the
//                          crop).
//   no crop (bit 2 clear): the sample is copied (mirrored where bit 0 is set).
//   C = 1                : a mask plane: v != 0 is read as 255 and result != 0 is written as 1.
// Every index the kernel forms comes from the descriptor, and every descriptor field and table row is checked on the host, from the
// host copy of the same words, before anything is enqueued. No atomics.
#include "haff_common.h"

#define HAFF_CROP_MAX_PIXELS (1L << 24)   // as the other augmentation kernels
#define HAFF_CROP_MAX_TAPS 17             // bicubic at a 4-fold down-scale: ceil(2 * 4) * 2 + 1
#define HAFF_CROP_GEOM 12                 // words per sample: x0 y0 cw ch px py S flags | htab hks vtab vks
#define HAFF_CROP_TW 64
#define HAFF_CROP_TH 16
#define HAFF_CROP_MAX_ROWS 96             // source rows of one tile's 16 output rows

namespace {

__device__ __forceinline__ int clip8(int v) { return min(max(v, 0), 255); }

template <int C>
__global__ __launch_bounds__(256) void crop_resample_kernel(const unsigned char* in, unsigned char* out, int H, int W,
                                                            const int* desc) {
  __shared__ unsigned char inter[HAFF_CROP_MAX_ROWS][HAFF_CROP_TW * C];
  const int b = (int)blockIdx.z;
  const int* g = desc + b * HAFF_CROP_GEOM;
  const int flags = g[7];
  const bool mirror = flags & 1;
  const long plane = (long)H * W * C;
  const unsigned char* src = in + plane * b;
  unsigned char* dst = out + plane * b;
  const int ox0 = (int)blockIdx.x * HAFF_CROP_TW, oy0 = (int)blockIdx.y * HAFF_CROP_TH;
  const int tw = min(HAFF_CROP_TW, W - ox0), th = min(HAFF_CROP_TH, H - oy0);

  if (!(flags & 4)) {                                             // uniform per block: the sample is copied through
    for (int i = (int)threadIdx.x; i < th * tw; i += 256) {
      const int r = i / tw, x = ox0 + i - r * tw, y = oy0 + r;
      const unsigned char* s = src + ((long)y * W + (mirror ? W - 1 - x : x)) * C;
      unsigned char* d = dst + ((long)y * W + x) * C;
#pragma unroll
      for (int c = 0; c < C; ++c) d[c] = C == 1 ? (unsigned char)(s[c] != 0) : s[c];
    }
    return;
  }

  const int x0 = g[0], y0 = g[1], cw = g[2], ch = g[3], px = g[4], py = g[5];
  const int* ht = desc + g[8];
  const int hs = 2 + g[9];
  const int* vt = desc + g[10];
  const int vs = 2 + g[11];
  // rows of Q the tile's output rows read: first and end are non-decreasing down the table (the host checked this tile's span)
  const int r_lo = vt[oy0 * vs];
  const int r_hi = vt[(oy0 + th - 1) * vs] + vt[(oy0 + th - 1) * vs + 1];
  const int nrows = r_hi - r_lo;

  // horizontal pass: lane = one pixel of the intermediate (a Q row, an output column), the taps are neighbouring bytes of one row
  for (int i = (int)threadIdx.x; i < nrows * tw; i += 256) {
    const int r = i / tw, xx = i - r * tw;
    const int sy = r_lo + r - py;                                 // the box's row; outside it Q is black
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = 1 << 21;
    if (sy >= 0 && sy < ch) {
      const int* hrow = ht + (ox0 + xx) * hs;
      const int first = hrow[0];
      const int t_lo = max(0, px - first), t_hi = min(hrow[1], px + cw - first);   // the taps inside the pasted window
      const unsigned char* row = src + (long)(y0 + sy) * W * C;
      for (int t = t_lo; t < t_hi; ++t) {
        const int bx = x0 + first + t - px;                       // in [x0, x0 + cw)
        const unsigned char* p = row + (mirror ? W - 1 - bx : bx) * C;
        const int k = hrow[2 + t];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] += (C == 1 ? (p[c] ? 255 : 0) : (int)p[c]) * k;
      }
    }
#pragma unroll
    for (int c = 0; c < C; ++c) inter[r][xx * C + c] = (unsigned char)clip8(acc[c] >> 22);
  }
  __syncthreads();

  // vertical pass: lane = one output byte; a wave reads 64 neighbouring bytes of one LDS row per tap
  const int rb = tw * C;
  for (int i = (int)threadIdx.x; i < th * rb; i += 256) {
    const int r = i / rb, j = i - r * rb;
    const int* vrow = vt + (oy0 + r) * vs;
    const int first = vrow[0] - r_lo, n = vrow[1];
    int acc = 1 << 21;
    for (int t = 0; t < n; ++t) acc += (int)inter[first + t][j] * vrow[2 + t];
    const int v = clip8(acc >> 22);
    dst[((long)(oy0 + r) * W + ox0) * C + j] = (unsigned char)(C == 1 ? (v != 0) : v);
  }
}

// one axis table of n_out rows (first, count, k[ks]) at word `off` of the descriptor: inside it, and every row inside [0, S)
bool crop_table_ok(const int* desc, long words, int off, int ks, int n_out, int S) {
  if (ks < 1 || ks > HAFF_CROP_MAX_TAPS || off < 0 || (long)off + (long)n_out * (2 + ks) > words) return false;
  const int* t = desc + off;
  for (int i = 0; i < n_out; ++i) {
    const int first = t[i * (2 + ks)], n = t[i * (2 + ks) + 1];
    if (first < 0 || n < 0 || n > ks || first + n > S) return false;
  }
  return true;
}

// the rows of the intermediate a tile of HAFF_CROP_TH output rows reads, as the kernel takes them: [first of its first row, end of
// its last row) must hold every row's taps and fit the LDS
bool crop_tiles_ok(const int* t, int ks, int H) {
  const int st = 2 + ks;
  for (int y0 = 0; y0 < H; y0 += HAFF_CROP_TH) {
    const int y1 = (y0 + HAFF_CROP_TH < H ? y0 + HAFF_CROP_TH : H) - 1;
    const int lo = t[y0 * st], hi = t[y1 * st] + t[y1 * st + 1];
    if (hi - lo < 0 || hi - lo > HAFF_CROP_MAX_ROWS) return false;
    for (int y = y0; y <= y1; ++y)
      if (t[y * st] < lo || t[y * st] + t[y * st + 1] > hi) return false;
  }
  return true;
}

}  // namespace

extern "C" int haff_crop_resample_u8(const void* in, void* out, int B, int H, int W, int C, const int* desc_host, const int* desc_dev,
                                     long desc_words, void* stream) {
  if (!in || !out || !desc_host || !desc_dev || B <= 0 || B > 65535 || H <= 0 || W <= 0 || (C != 1 && C != 3)) return HAFF_ERR_BAD_ARG;
  if (!haff_aligned(desc_host, 4) || !haff_aligned(desc_dev, 4) || desc_words < (long)B * HAFF_CROP_GEOM) return HAFF_ERR_BAD_ARG;
  if ((long)H * W > HAFF_CROP_MAX_PIXELS || (H + HAFF_CROP_TH - 1) / HAFF_CROP_TH > 65535) return HAFF_ERR_UNSUPPORTED;
  const long bytes = (long)B * H * W * C;
  const long gap = (const char*)out - (const char*)in;
  if (gap < bytes && -gap < bytes) return HAFF_ERR_BAD_ARG;      // out of place: the mirror reads what it would overwrite
  for (int b = 0; b < B; ++b) {
    const int* g = desc_host + (long)b * HAFF_CROP_GEOM;
    if (g[7] & ~5) return HAFF_ERR_BAD_ARG;
    if (!(g[7] & 4)) continue;
    const int x0 = g[0], y0 = g[1], cw = g[2], ch = g[3], px = g[4], py = g[5], S = g[6];
    if (x0 < 0 || y0 < 0 || cw < 1 || ch < 1 || cw > W || ch > H || x0 > W - cw || y0 > H - ch) return HAFF_ERR_BAD_ARG;
    if (S != (cw > ch ? cw : ch) || px < 0 || py < 0 || px > S - cw || py > S - ch) return HAFF_ERR_BAD_ARG;
    if (S > 4L * W || S > 4L * H) return HAFF_ERR_UNSUPPORTED;   // more than 17 taps: the caller's host route
    if (!crop_table_ok(desc_host, desc_words, g[8], g[9], W, S) || !crop_table_ok(desc_host, desc_words, g[10], g[11], H, S))
      return HAFF_ERR_BAD_ARG;
    if (!crop_tiles_ok(desc_host + g[10], g[11], H)) return HAFF_ERR_UNSUPPORTED;
  }
  const dim3 grid((unsigned)((W + HAFF_CROP_TW - 1) / HAFF_CROP_TW), (unsigned)((H + HAFF_CROP_TH - 1) / HAFF_CROP_TH), (unsigned)B);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (C == 3)
    hipLaunchKernelGGL((crop_resample_kernel<3>), grid, dim3(256), 0, s, (const unsigned char*)in, (unsigned char*)out, H, W, desc_dev);
  else
    hipLaunchKernelGGL((crop_resample_kernel<1>), grid, dim3(256), 0, s, (const unsigned char*)in, (unsigned char*)out, H, W, desc_dev);
  return haff_check_launch();
}
