// Training augmentation on the device (train_ds.py --aug_flip / --aug_jitter with --device_ingest): the two offline augmentations of
// the 2HANDS training set (2HANDS/scripts/data_augmentation/horizontal_flip.py and apply_jitter.py) applied per sample to the uint8
// frames in HBM, byte for byte what Pillow gives:
//
//   jitter = ImageEnhance.Brightness(im).enhance(fb) -> Contrast(..).enhance(fc) -> Color(..).enhance(fs) on the RGB frame, each an
//            Image.blend(degenerate, image, f):
//     L(r,g,b)       = (19595 r + 38470 g + 7471 b + 32768) >> 16                                  (ImagingConvert rgb2l)
//     blend(d, i, f) = clip8(trunc(fl32(fl32(d) + fl32(f * fl32(i - d)))))                         product and sum round SEPARATELY
//     p1 = blend(0, p, fb);  S = sum of L(p1) over the frame, m = (2 S + n) div 2 n;  p2 = blend(m, p1, fc);  p3 = blend(L(p2), p2, fs)
//   flip   = Image.transpose(FLIP_LEFT_RIGHT): the PIXELS of every row reversed.
//   The jitter is pointwise apart from the frame mean m, which a mirror keeps, so the two commute and one pass does both.
//
//   haff_jitter_stats_u8 : S per jittered frame. Each lane takes 16 pixels (48 bytes, three 16-byte loads) of the flat frame per step,
//                          a block adds its lanes' integer partials (shuffles, then LDS) and issues ONE 64-bit atomicAdd: integer
//                          sums, so the result does not depend on the order. The slots are zeroed by a memset in front of the kernel.
//   haff_augment_u8      : out of place, one pass, 3 n bytes read and 3 n written per frame. A work item is 16 pixels of one row
//                          (or the row's last W % 16 pixels, which move byte by byte); with the mirror the item's 48 bytes land at
//                          the mirrored position with their pixels in reverse order, so loads and stores are both whole 16-byte pieces.
//   haff_flip_planes_u8  : the mirror for single-channel planes (the filled masks), 16 bytes per lane reversed with byte swaps.
// Rows of 3 W bytes start at any address, so the 16-byte accesses are unaligned ones (global memory takes them on gfx950).
// Every size and pointer is checked on the host before anything is enqueued; a kernel indexes only with H, W and B.
#include "haff_common.h"

#define HAFF_AUG_MAX_PIXELS (1L << 24)   // H * W per frame: S < 2^32 and (2 S + n) / 2 n is Pillow's int(mean + 0.5)

namespace {

struct Jitter {
  float fb, fc, fs;
  int mean;
};

// Pillow's C rounds the product to fp32 before the sum. The build contracts across statements (-ffp-contract=fast, in the backend,
// whatever a pragma says), so the product passes through the empty fence nf4_dequant_lora_kernel uses: no fused multiply-add here.
__device__ __forceinline__ int blend8(int d, int i, float f) {
  float prod = __fmul_rn(f, (float)(i - d));
  asm("" : "+v"(prod));   // not volatile: the value only has to be opaque, the 48 blends of a lane's piece may still interleave
  const float t = __fadd_rn((float)d, prod);
  return t <= 0.f ? 0 : (t >= 255.f ? 255 : (int)t);
}

__device__ __forceinline__ int luma8(int r, int g, int b) { return (19595 * r + 38470 * g + 7471 * b + 32768) >> 16; }

__device__ __forceinline__ void jitter_pixel(int c[3], const Jitter& j) {
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = blend8(j.mean, blend8(0, c[k], j.fb), j.fc);
  const int l = luma8(c[0], c[1], c[2]);
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = blend8(l, c[k], j.fs);
}

struct Words12 { unsigned w[12]; };
struct Words4 { unsigned w[4]; };

// 16 RGB pixels (48 bytes at any address) -> 48 bytes; FLIP reverses the pixel order inside the piece
template <bool FLIP, bool JIT>
__device__ __forceinline__ void pixels16(const unsigned char* src, unsigned char* dst, const Jitter& j) {
  Words12 in, out;
  __builtin_memcpy(&in, src, 48);
#pragma unroll
  for (int k = 0; k < 12; ++k) out.w[k] = 0u;
#pragma unroll
  for (int p = 0; p < 16; ++p) {
    int c[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) c[k] = (int)((in.w[(3 * p + k) >> 2] >> (8 * ((3 * p + k) & 3))) & 255u);
    if (JIT) jitter_pixel(c, j);
    const int o = FLIP ? 15 - p : p;
#pragma unroll
    for (int k = 0; k < 3; ++k) out.w[(3 * o + k) >> 2] |= (unsigned)c[k] << (8 * ((3 * o + k) & 3));
  }
  __builtin_memcpy(dst, &out, 48);
}

template <bool FLIP, bool JIT>
__device__ __forceinline__ void augment_frame(const unsigned char* in, unsigned char* out, int H, int W, const Jitter& j) {
  const int cpr = (W + 15) >> 4;                                  // work items per row; the last one holds W - 16 (cpr - 1) pixels
  const int items = H * cpr;
  for (int it = (int)(blockIdx.x * blockDim.x + threadIdx.x); it < items; it += (int)(gridDim.x * blockDim.x)) {
    const int row = it / cpr, x0 = (it - row * cpr) << 4;
    const int npx = min(16, W - x0);
    const int xd = FLIP ? W - x0 - npx : x0;                      // where the item's pixels land
    const unsigned char* src = in + ((long)row * W + x0) * 3;
    unsigned char* dst = out + ((long)row * W + xd) * 3;
    if (npx == 16) {
      pixels16<FLIP, JIT>(src, dst, j);
    } else {
      for (int p = 0; p < npx; ++p) {
        int c[3] = {src[3 * p], src[3 * p + 1], src[3 * p + 2]};
        if (JIT) jitter_pixel(c, j);
        unsigned char* d = dst + 3 * (FLIP ? npx - 1 - p : p);
        d[0] = (unsigned char)c[0];
        d[1] = (unsigned char)c[1];
        d[2] = (unsigned char)c[2];
      }
    }
  }
}

// grid (blocks per frame, frames); flags / factors / sums are read per frame, uniformly by the whole block
__global__ __launch_bounds__(256) void augment_kernel(const unsigned char* in, unsigned char* out, int B, int H, int W, const int* flags,
                                                      const float* factors, const unsigned long long* sums) {
  const long n = (long)H * W;
  for (int b = (int)blockIdx.y; b < B; b += (int)gridDim.y) {
    const int fl = flags[b];
    const unsigned char* src = in + 3 * n * b;
    unsigned char* dst = out + 3 * n * b;
    Jitter j = {1.f, 1.f, 1.f, 0};
    if (fl & 2) {
      j.fb = factors[3 * b];
      j.fc = factors[3 * b + 1];
      j.fs = factors[3 * b + 2];
      j.mean = (int)((2ULL * sums[b] + (unsigned long long)n) / (2ULL * (unsigned long long)n));
    }
    switch (fl & 3) {
      case 0: augment_frame<false, false>(src, dst, H, W, j); break;
      case 1: augment_frame<true, false>(src, dst, H, W, j); break;
      case 2: augment_frame<false, true>(src, dst, H, W, j); break;
      default: augment_frame<true, true>(src, dst, H, W, j); break;
    }
  }
}

__global__ __launch_bounds__(256) void jitter_stats_kernel(const unsigned char* in, int B, int H, int W, const int* flags,
                                                           const float* factors, unsigned long long* sums) {
  __shared__ unsigned red[4];
  const int n = H * W;                                            // <= 2^24, checked by the caller
  const int chunks = (n + 15) >> 4;
  for (int b = (int)blockIdx.y; b < B; b += (int)gridDim.y) {
    if (!(flags[b] & 2)) continue;                                // uniform: the whole block skips the frame
    const float fb = factors[3 * b];
    const unsigned char* src = in + 3L * n * b;
    unsigned s = 0;                                               // a frame's whole sum is below 2^32
    for (int it = (int)(blockIdx.x * blockDim.x + threadIdx.x); it < chunks; it += (int)(gridDim.x * blockDim.x)) {
      const int p0 = it << 4;
      if (p0 + 16 <= n) {
        Words12 w;
        __builtin_memcpy(&w, src + 3L * p0, 48);
#pragma unroll
        for (int p = 0; p < 16; ++p) {
          int c[3];
#pragma unroll
          for (int k = 0; k < 3; ++k) c[k] = blend8(0, (int)((w.w[(3 * p + k) >> 2] >> (8 * ((3 * p + k) & 3))) & 255u), fb);
          s += (unsigned)luma8(c[0], c[1], c[2]);
        }
      } else {
        for (int p = p0; p < n; ++p) {
          const unsigned char* q = src + 3L * p;
          s += (unsigned)luma8(blend8(0, q[0], fb), blend8(0, q[1], fb), blend8(0, q[2], fb));
        }
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
      const unsigned long long t = (unsigned long long)red[0] + red[1] + red[2] + red[3];
      if (t) atomicAdd(&sums[b], t);
    }
    __syncthreads();                                              // the next frame rewrites red
  }
}

__global__ __launch_bounds__(256) void flip_planes_kernel(const unsigned char* in, unsigned char* out, int P, int H, int W,
                                                          const int* flags) {
  const int cpr = (W + 15) >> 4;
  const long items = (long)H * cpr;
  for (int pl = (int)blockIdx.y; pl < P; pl += (int)gridDim.y) {
    const bool flip = flags[pl] & 1;
    const unsigned char* src_p = in + (long)pl * H * W;
    unsigned char* dst_p = out + (long)pl * H * W;
    for (long it = (long)blockIdx.x * blockDim.x + threadIdx.x; it < items; it += (long)gridDim.x * blockDim.x) {
      const int row = (int)(it / cpr), x0 = (int)(it - (long)row * cpr) << 4;
      const int nb = min(16, W - x0);
      const unsigned char* src = src_p + (long)row * W + x0;
      unsigned char* dst = dst_p + (long)row * W + (flip ? W - x0 - nb : x0);
      if (nb == 16) {
        Words4 a, r;
        __builtin_memcpy(&a, src, 16);
        if (flip) {
#pragma unroll
          for (int k = 0; k < 4; ++k) r.w[k] = __builtin_bswap32(a.w[3 - k]);
        } else {
          r = a;
        }
        __builtin_memcpy(dst, &r, 16);
      } else {
        for (int k = 0; k < nb; ++k) dst[flip ? nb - 1 - k : k] = src[k];
      }
    }
  }
}


// blocks of 256 lanes over `items` work items of one frame / plane: at most 1024 per frame, the rest by grid stride
inline dim3 aug_grid(long items, int count) {
  long bx = (items + 255) / 256;
  return dim3((unsigned)(bx < 1 ? 1 : (bx > 1024 ? 1024 : bx)), (unsigned)(count > 65535 ? 65535 : count));
}

}  // namespace

extern "C" int haff_jitter_stats_u8(const void* frames, int B, int H, int W, const int* flags, const float* factors, void* sums,
                                    void* stream) {
  if (!frames || !flags || !factors || !sums || B <= 0 || H <= 0 || W <= 0) return HAFF_ERR_BAD_ARG;
  if (!haff_aligned(flags, 4) || !haff_aligned(factors, 4) || !haff_aligned(sums, 8)) return HAFF_ERR_BAD_ARG;
  if ((long)H * W > HAFF_AUG_MAX_PIXELS) return HAFF_ERR_UNSUPPORTED;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(sums, 0, (size_t)B * 8, s) != hipSuccess) return HAFF_ERR_LAUNCH;
  const long chunks = ((long)H * W + 15) / 16;
  hipLaunchKernelGGL(jitter_stats_kernel, aug_grid(chunks, B), dim3(256), 0, s, (const unsigned char*)frames, B, H, W, flags, factors,
                     (unsigned long long*)sums);
  return haff_check_launch();
}

extern "C" int haff_augment_u8(const void* in, void* out, int B, int H, int W, const int* flags, const float* factors, const void* sums,
                               void* stream) {
  if (!in || !out || !flags || !factors || !sums || B <= 0 || H <= 0 || W <= 0) return HAFF_ERR_BAD_ARG;
  if (!haff_aligned(flags, 4) || !haff_aligned(factors, 4) || !haff_aligned(sums, 8)) return HAFF_ERR_BAD_ARG;
  if ((long)H * W > HAFF_AUG_MAX_PIXELS) return HAFF_ERR_UNSUPPORTED;
  const long bytes = 3L * H * W * B;
  const long gap = (const char*)out - (const char*)in;
  if (gap < bytes && -gap < bytes) return HAFF_ERR_BAD_ARG;      // out == in, or any overlap: the mirror reads what it would overwrite
  const long items = (long)H * ((W + 15) / 16);
  hipLaunchKernelGGL(augment_kernel, aug_grid(items, B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), (const unsigned char*)in,
                     (unsigned char*)out, B, H, W, flags, factors, (const unsigned long long*)sums);
  return haff_check_launch();
}

extern "C" int haff_flip_planes_u8(const void* in, void* out, int P, int H, int W, const int* flags, void* stream) {
  if (!in || !out || !flags || P <= 0 || H <= 0 || W <= 0 || !haff_aligned(flags, 4)) return HAFF_ERR_BAD_ARG;
  const long bytes = (long)P * H * W;
  const long gap = (const char*)out - (const char*)in;
  if (gap < bytes && -gap < bytes) return HAFF_ERR_BAD_ARG;
  const long items = (long)H * ((W + 15) / 16);
  hipLaunchKernelGGL(flip_planes_kernel, aug_grid(items, P), dim3(256), 0, reinterpret_cast<hipStream_t>(stream),
                     (const unsigned char*)in, (unsigned char*)out, P, H, W, flags);
  return haff_check_launch();
}
