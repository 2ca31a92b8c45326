// NF4 (4-bit NormalFloat) language-model weights for the fp16 inference mode: load-time quantisation, dequantisation and the
// weight-streaming product of decode-sized M on the packed weights; and for NF4 fine-tuning (QLoRA), whose frozen products
// dequantise row-major for the forward and TRANSPOSED (nf4_dequant_t_kernel) for the dX products.
//
// The format is the one bitsandbytes' `load_in_4bit=True, bnb_4bit_quant_type="nf4", bnb_4bit_use_double_quant=True` gives the
// reference (2Haff/inference.py:133-146), restated in 2handedafforder_amd/quant.py, stored ROW-LOCAL so that row reorders of a
// weight (q|k|v concatenation, the [gate x16 | up x16] SwiGLU interleave, the RoPE row permutation) stay row reorders:
//   packed  uint8 [N][K/2]   code of W[n][k] in byte k/2, even k in the HIGH nibble
//   absmax  fp32  [N][K/64]  the DEQUANTISED block absmax (after the double-quantisation round trip), K % 64 == 0
// A weight enters every product as f16_rn(NF4[code] * absmax): one fp32 multiply, one rounding.
//
// gemm_nf4_kernel follows gemm_skinny_kernel (gemm_bf16.hip): one workgroup per 16 * NT weight rows, KW waves splitting K into
// contiguous ranges of 64-deep blocks, the activation rows (L2-resident) as the MFMA B operand, v_mfma_f32_16x16x32_f16, the KW
// partial tiles summed in LDS in wave order (no atomics: repeat runs are bitwise equal). Lane (fr, fh) of a weight tile holds
// row fr, weights 16 fh .. 16 fh + 15 of a 64-block: 8 packed bytes and the block's absmax. A byte (two codes) is looked up in
// a 256-entry LDS table of fp32 pairs {NF4[hi], NF4[lo]} (one ds_read_b64 per two weights), scaled by absmax with one packed
// multiply and rounded to f16 with one packed convert.
#include "haff_common.h"
#include "gemm_quant.h"

#include <type_traits>

namespace {

// bitsandbytes' NF4 code values (index 7 is 0)
__constant__ float kNF4[16] = {
    -1.0f, -0.6961928009986877f, -0.5250730514526367f, -0.39491748809814453f, -0.28444138169288635f, -0.18477343022823334f,
    -0.09105003625154495f, 0.0f, 0.07958029955625534f, 0.16093020141124725f, 0.24611230194568634f, 0.33791524171829224f,
    0.44070982933044434f, 0.5626170039176941f, 0.7229568362236023f, 1.0f};

// the signed 8-bit "dynamic" map of the double quantisation (create_dynamic_map(signed=True) as restated in quant.py:
// 7 decades of 2^i interval means each side, then 0 and +1; float32, sorted; index 127 is 0). tests/test_nf4_cpu.py checks
// these literals against quant.py.
__constant__ float kDynMap[256] = {
    -0x1.fc6666p-1f, -0x1.f53334p-1f, -0x1.eep-1f, -0x1.e6ccccp-1f, -0x1.df999ap-1f, -0x1.d86666p-1f,
    -0x1.d13334p-1f, -0x1.cap-1f, -0x1.c2ccccp-1f, -0x1.bb999ap-1f, -0x1.b46666p-1f, -0x1.ad3334p-1f,
    -0x1.a6p-1f, -0x1.9eccccp-1f, -0x1.97999ap-1f, -0x1.906666p-1f, -0x1.893334p-1f, -0x1.82p-1f,
    -0x1.7accccp-1f, -0x1.73999ap-1f, -0x1.6c6668p-1f, -0x1.653334p-1f, -0x1.5ep-1f, -0x1.56ccccp-1f,
    -0x1.4f999ap-1f, -0x1.486668p-1f, -0x1.413334p-1f, -0x1.3ap-1f, -0x1.32ccccp-1f, -0x1.2b999ap-1f,
    -0x1.246668p-1f, -0x1.1d3334p-1f, -0x1.16p-1f, -0x1.0eccccp-1f, -0x1.079998p-1f, -0x1.006666p-1f,
    -0x1.f26664p-2f, -0x1.e4p-2f, -0x1.d59998p-2f, -0x1.c73334p-2f, -0x1.b8ccccp-2f, -0x1.aa6666p-2f,
    -0x1.9cp-2f, -0x1.8d9998p-2f, -0x1.7f3334p-2f, -0x1.70ccccp-2f, -0x1.626666p-2f, -0x1.54p-2f,
    -0x1.459998p-2f, -0x1.373334p-2f, -0x1.28ccccp-2f, -0x1.1a6668p-2f, -0x1.0cp-2f, -0x1.fb3332p-3f,
    -0x1.de6666p-3f, -0x1.c1999ap-3f, -0x1.a4ccccp-3f, -0x1.88p-3f, -0x1.6b3334p-3f, -0x1.4e6666p-3f,
    -0x1.31999ap-3f, -0x1.14ccccp-3f, -0x1.fp-4f, -0x1.b66668p-4f, -0x1.93d70ap-4f, -0x1.8851eep-4f,
    -0x1.7ccccep-4f, -0x1.7147aep-4f, -0x1.65c29p-4f, -0x1.5a3d7p-4f, -0x1.4eb854p-4f, -0x1.433334p-4f,
    -0x1.37ae14p-4f, -0x1.2c28f6p-4f, -0x1.20a3d6p-4f, -0x1.151ebap-4f, -0x1.09999ap-4f, -0x1.fc28f6p-5f,
    -0x1.e51ebap-5f, -0x1.ce147ap-5f, -0x1.b70a3ep-5f, -0x1.ap-5f, -0x1.88f5c2p-5f, -0x1.71eb86p-5f,
    -0x1.5ae146p-5f, -0x1.43d70ap-5f, -0x1.2ccccep-5f, -0x1.15c29p-5f, -0x1.fd70a4p-6f, -0x1.cf5c2ap-6f,
    -0x1.a147aep-6f, -0x1.733334p-6f, -0x1.451ebap-6f, -0x1.170a3ep-6f, -0x1.d1eb86p-7f, -0x1.75c29p-7f,
    -0x1.3e76c8p-7f, -0x1.2c083p-7f, -0x1.19999ap-7f, -0x1.072b02p-7f, -0x1.e978d4p-8f, -0x1.c49ba6p-8f,
    -0x1.9fbe76p-8f, -0x1.7ae148p-8f, -0x1.56041ap-8f, -0x1.3126e8p-8f, -0x1.0c49bap-8f, -0x1.ced914p-9f,
    -0x1.851eb8p-9f, -0x1.3b645ap-9f, -0x1.e353f8p-10f, -0x1.4fdf3ap-10f, -0x1.eecbfep-11f, -0x1.b3d07cp-11f,
    -0x1.78d5p-11f, -0x1.3dd982p-11f, -0x1.02de02p-11f, -0x1.8fc506p-12f, -0x1.19ce0ap-12f, -0x1.47ae16p-13f,
    -0x1.743e96p-14f, -0x1.15df66p-14f, -0x1.6f0068p-15f, -0x1.64840cp-16f, -0x1.040bfep-17f, -0x1.b43528p-19f,
    -0x1.27476ep-21f, 0x0.0p+0f, 0x1.27476ep-21f, 0x1.b43528p-19f, 0x1.040bfep-17f, 0x1.64840cp-16f,
    0x1.6f0068p-15f, 0x1.15df66p-14f, 0x1.743e96p-14f, 0x1.47ae16p-13f, 0x1.19ce0ap-12f, 0x1.8fc506p-12f,
    0x1.02de02p-11f, 0x1.3dd982p-11f, 0x1.78d5p-11f, 0x1.b3d07cp-11f, 0x1.eecbfep-11f, 0x1.4fdf3ap-10f,
    0x1.e353f8p-10f, 0x1.3b645ap-9f, 0x1.851eb8p-9f, 0x1.ced914p-9f, 0x1.0c49bap-8f, 0x1.3126e8p-8f,
    0x1.56041ap-8f, 0x1.7ae148p-8f, 0x1.9fbe76p-8f, 0x1.c49ba6p-8f, 0x1.e978d4p-8f, 0x1.072b02p-7f,
    0x1.19999ap-7f, 0x1.2c083p-7f, 0x1.3e76c8p-7f, 0x1.75c29p-7f, 0x1.d1eb86p-7f, 0x1.170a3ep-6f,
    0x1.451ebap-6f, 0x1.733334p-6f, 0x1.a147aep-6f, 0x1.cf5c2ap-6f, 0x1.fd70a4p-6f, 0x1.15c29p-5f,
    0x1.2ccccep-5f, 0x1.43d70ap-5f, 0x1.5ae146p-5f, 0x1.71eb86p-5f, 0x1.88f5c2p-5f, 0x1.ap-5f,
    0x1.b70a3ep-5f, 0x1.ce147ap-5f, 0x1.e51ebap-5f, 0x1.fc28f6p-5f, 0x1.09999ap-4f, 0x1.151ebap-4f,
    0x1.20a3d6p-4f, 0x1.2c28f6p-4f, 0x1.37ae14p-4f, 0x1.433334p-4f, 0x1.4eb854p-4f, 0x1.5a3d7p-4f,
    0x1.65c29p-4f, 0x1.7147aep-4f, 0x1.7ccccep-4f, 0x1.8851eep-4f, 0x1.93d70ap-4f, 0x1.b66668p-4f,
    0x1.fp-4f, 0x1.14ccccp-3f, 0x1.31999ap-3f, 0x1.4e6666p-3f, 0x1.6b3334p-3f, 0x1.88p-3f,
    0x1.a4ccccp-3f, 0x1.c1999ap-3f, 0x1.de6666p-3f, 0x1.fb3332p-3f, 0x1.0cp-2f, 0x1.1a6668p-2f,
    0x1.28ccccp-2f, 0x1.373334p-2f, 0x1.459998p-2f, 0x1.54p-2f, 0x1.626666p-2f, 0x1.70ccccp-2f,
    0x1.7f3334p-2f, 0x1.8d9998p-2f, 0x1.9cp-2f, 0x1.aa6666p-2f, 0x1.b8ccccp-2f, 0x1.c73334p-2f,
    0x1.d59998p-2f, 0x1.e4p-2f, 0x1.f26664p-2f, 0x1.006666p-1f, 0x1.079998p-1f, 0x1.0eccccp-1f,
    0x1.16p-1f, 0x1.1d3334p-1f, 0x1.246668p-1f, 0x1.2b999ap-1f, 0x1.32ccccp-1f, 0x1.3ap-1f,
    0x1.413334p-1f, 0x1.486668p-1f, 0x1.4f999ap-1f, 0x1.56ccccp-1f, 0x1.5ep-1f, 0x1.653334p-1f,
    0x1.6c6668p-1f, 0x1.73999ap-1f, 0x1.7accccp-1f, 0x1.82p-1f, 0x1.893334p-1f, 0x1.906666p-1f,
    0x1.97999ap-1f, 0x1.9eccccp-1f, 0x1.a6p-1f, 0x1.ad3334p-1f, 0x1.b46666p-1f, 0x1.bb999ap-1f,
    0x1.c2ccccp-1f, 0x1.cap-1f, 0x1.d13334p-1f, 0x1.d86666p-1f, 0x1.df999ap-1f, 0x1.e6ccccp-1f,
    0x1.eep-1f, 0x1.f53334p-1f, 0x1.fc6666p-1f, 0x1p+0f};

// Index of the nearest table value to x: the number of fp32 midpoints of neighbouring values that x exceeds. A value exactly on
// a midpoint takes the LOWER index; x = +-0 takes the index of 0.
template <int N>
__device__ __forceinline__ int nearest_code(const float* tab, float x) {
  int lo = 0, hi = N - 1;   // count of midpoints m_i = (tab[i] + tab[i + 1]) / 2, i < N - 1, with x > m_i: binary search
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const float m = (tab[mid] + tab[mid + 1]) * 0.5f;
    if (x > m) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// Pass 1: thread = 8 consecutive weights of one row, 8 lanes = one 64-block. Block absmax (fp32 max |w|), the codes of
// w * (1/absmax) (correctly rounded reciprocal, one rounding per product; absmax == 0: every code is 7), packed to
// dst row map[n] (or n); the raw absmax in SOURCE order to amax_src (the double quantisation blocks run over it flat).
__global__ __launch_bounds__(256) void nf4_codes_kernel(const bf16_t* __restrict__ W, long ldw, int N, int K, const int* row_map,
                                                        unsigned char* __restrict__ packed, float* __restrict__ amax_src) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int g8 = K >> 3;
  if (gid >= (long)N * g8) return;   // (N * g8 is a multiple of 8: whole groups of 8 lanes leave together)
  const int n = (int)(gid / g8), g = (int)(gid % g8);
  float v[8];
  load8(reinterpret_cast<const f16_t*>(W) + (long)n * ldw + 8 * g, v);
  float a = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) a = fmaxf(a, fabsf(v[i]));
  a = fmaxf(a, __shfl_xor(a, 1, 64));
  a = fmaxf(a, __shfl_xor(a, 2, 64));
  a = fmaxf(a, __shfl_xor(a, 4, 64));
  const float inv = a > 0.f ? __fdiv_rn(1.0f, a) : 0.f;
  unsigned word = 0;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const unsigned c = (unsigned)nearest_code<16>(kNF4, __fmul_rn(v[i], inv));
    word |= c << (i & 1 ? 8 * (i >> 1) : 8 * (i >> 1) + 4);   // even k: high nibble of its byte
  }
  const long dst = row_map ? row_map[n] : n;
  *reinterpret_cast<unsigned*>(packed + dst * (K >> 1) + 4 * g) = word;
  if ((g & 7) == 0) amax_src[(long)n * (K >> 6) + (g >> 3)] = a;
}

// Pass 2: the mean of the absmax values, summed in double in a fixed order (one workgroup: thread t takes t, t + 256, ...,
// then a fixed tree), rounded once to fp32.
__global__ __launch_bounds__(256) void nf4_offset_kernel(const float* __restrict__ amax_src, long nb, float* offset) {
  __shared__ double part[256];
  double s = 0.0;
  for (long i = threadIdx.x; i < nb; i += 256) s += (double)amax_src[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) *offset = (float)(part[0] / (double)nb);
}

// Pass 3: the absmax values the products use, to dst row map[n]. double_quant: blocks of 256 consecutive (flat, source
// order) values a - offset, absmax2 = their max |.|, code = nearest dynamic-map value of (a - offset) * (1/absmax2), value
// map[code] * absmax2 + offset (a multiply and an add, each rounded: no fused multiply-add); otherwise the raw absmax.
__global__ __launch_bounds__(256) void nf4_absmax_kernel(const float* __restrict__ amax_src, long nb, int kb, const int* row_map,
                                                         int double_quant, const float* offset, float* __restrict__ absmax) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  float val = i < nb ? amax_src[i] : 0.f;
  if (double_quant) {
    const float off = *offset;
    const float d = i < nb ? __fsub_rn(val, off) : 0.f;
    __shared__ float red[4];
    float m = wave_max(fabsf(d));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const float inv = m > 0.f ? __fdiv_rn(1.0f, m) : 0.f;
    const int c = nearest_code<256>(kDynMap, __fmul_rn(d, inv));
    float prod = __fmul_rn(kDynMap[c], m);
    asm volatile("" : "+v"(prod));   // the build contracts across statements (-ffp-contract=fast): keep the multiply's rounding
    val = __fadd_rn(prod, off);
  }
  if (i >= nb) return;
  const long n = i / kb;
  absmax[(row_map ? (long)row_map[n] : n) * kb + i % kb] = val;
}

// f16_rn(NF4[code] * absmax) of stored row n to out row map[n] (or n); thread = 8 weights
__global__ __launch_bounds__(256) void nf4_dequant_kernel(const unsigned char* __restrict__ packed, const float* __restrict__ absmax,
                                                          int N, int K, const int* row_map, bf16_t* out, long ldo) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int g8 = K >> 3;
  if (gid >= (long)N * g8) return;
  const int n = (int)(gid / g8), g = (int)(gid % g8);
  const unsigned word = *reinterpret_cast<const unsigned*>(packed + (long)n * (K >> 1) + 4 * g);
  const float a = absmax[(long)n * (K >> 6) + (g >> 3)];
  float v[8];
#pragma unroll
  for (int i = 0; i < 8; ++i) v[i] = __fmul_rn(kNF4[(word >> (i & 1 ? 8 * (i >> 1) : 8 * (i >> 1) + 4)) & 15u], a);
  const long dst = row_map ? row_map[n] : n;
  store8(reinterpret_cast<f16_t*>(out) + dst * ldo + 8 * g, v);
}

// nf4_dequant_kernel with the rank-8 update of unmerged LoRA adapters folded into the same pass (serving adapters fitted on the NF4
// base; prefill-sized products):
//   out[map[n]][k] = f16_rn(fl32(d + fl32(s * u))),  d = fl32(NF4[code] * absmax),
//   u_0 = 0, u_{j+1} = fl32(u_j + B[n][j] * A[8 seg(n) + j][k]), j = 0..7 in that order (an f16 x f16 product is exact in fp32, so
//   one fused multiply-add per step rounds exactly once, as written), seg(n) = (n / seg_rows) % nseg.
// Thread = 8 consecutive k of 8 consecutive stored rows (seg_rows % 16 == 0: one segment): its 8 x 8 block of A_cat is read once
// (L2-resident: 16 nseg K bytes in all) and serves the 8 rows, so the kernel moves the plain dequantisation's HBM bytes plus N K / 4
// bytes of L2 reads. Lanes walk k: the code words of a wave are 256 contiguous bytes of a row, its stores 1 KiB of one.
__global__ __launch_bounds__(256) void nf4_dequant_lora_kernel(const unsigned char* __restrict__ packed, const float* __restrict__ absmax,
                                                               int N, int K, const int* row_map, f16_t* out, long ldo,
                                                               const f16_t* __restrict__ A, long lda, const f16_t* __restrict__ B,
                                                               int nseg, int seg_rows, float scale) {
  const long gid = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int g8 = K >> 3;
  const int groups = (N + 7) >> 3;
  if (gid >= (long)groups * g8) return;
  const int n0 = (int)(gid / g8) * 8, g = (int)(gid % g8);
  const int seg = (n0 / seg_rows) % nseg;
  float a[8][8];
#pragma unroll
  for (int j = 0; j < 8; ++j) load8(A + (long)(8 * seg + j) * lda + 8 * g, a[j]);
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int n = min(n0 + i, N - 1);   // rows past N: re-read, skipped at the store (no branch between the rows' loads)
    const unsigned word = *reinterpret_cast<const unsigned*>(packed + (long)n * (K >> 1) + 4 * g);
    const float am = absmax[(long)n * (K >> 6) + (g >> 3)];
    float b[8];
    load8(B + (long)n * 8, b);
    float v[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float d = __fmul_rn(kNF4[(word >> (e & 1 ? 8 * (e >> 1) : 8 * (e >> 1) + 4)) & 15u], am);
      float u = 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j) u = __fmaf_rn(b[j], a[j][e], u);
      float su = __fmul_rn(scale, u);
      asm volatile("" : "+v"(d), "+v"(su));   // the build contracts across statements (-ffp-contract=fast): keep both products' roundings
      float o = __fadd_rn(d, su);
      asm volatile("" : "+v"(o));             // ... and the sum's: rounded to fp32 first, then to f16
      v[e] = o;
    }
    const long dst = row_map ? row_map[n] : n;
    if (n0 + i < N) store8(out + dst * ldo + 8 * g, v);
  }
}

typedef float nf4_f2 __attribute__((ext_vector_type(2)));

// The transposed dequantisation (NF4 fine-tuning: the f16 W^T of a dX product, written straight from the codes):
//   out_t[k][map[n]] = f16_rn(NF4[code(n, k)] * absmax(n, k / 64)),   columns N .. roundup(N, 8) - 1 zero.
// Pure data movement: N K / 2 code bytes and N K / 64 floats in, 2 K Np bytes out; the bound is HBM.
// One workgroup = 64 stored rows x 256 k through a [256 k][64 n] f16 LDS image (32 KiB).
//   fill: lane (row l / 8, piece l % 8) reads 16 B of codes (32 k of one row; 8 lanes = 128 contiguous bytes of the row) and the
//     block absmax, looks each byte up in the LDS table of {NF4[hi], NF4[lo]} pairs, and writes 32 f16 down a column of the
//     image. Piece p lands in image rows 32 p .. 32 p + 31 with its columns ROTATED by 8 p: at one step the wave's 64 lanes
//     (8 rows x 8 pieces) then touch all 32 LDS banks instead of the four an unrotated 128-B image row would give them.
//   drain: lane (k row l / 8, chunk l % 8) reads 8 consecutive columns (one ds_read_b128, the rotation keeps 8-column chunks
//     whole) and stores 16 B; 8 lanes = 128 contiguous bytes of an output row.
// A row_map is honoured per 8-column chunk: a chunk whose 8 stored rows go to 8 consecutive, 8-aligned columns (every chunk of
// the RoPE permutation and of the [gate x16 | up x16] interleave) keeps its 16-B store; any other chunk stores element by element.
constexpr int kT_N = 64, kT_K = 256;

__global__ __launch_bounds__(256) void nf4_dequant_t_kernel(const unsigned char* __restrict__ packed, const float* __restrict__ absmax,
                                                            int N, int K, const int* __restrict__ row_map, f16_t* out, long ldo) {
  __shared__ __attribute__((aligned(16))) f16_t tile[kT_K * kT_N];
  __shared__ nf4_f2 tab[256];
  const int tid = threadIdx.x;
  tab[tid] = nf4_f2{kNF4[tid >> 4], kNF4[tid & 15]};
  const int k0 = blockIdx.x * kT_K, n0 = blockIdx.y * kT_N;
  const int Np = (N + 7) & ~7;
  __syncthreads();
  {
    const int p = tid & 7;                 // 32 k of the tile
    const int kp = k0 + 32 * p;
#pragma unroll
    for (int it = 0; it < 2; ++it) {
      const int nl = (tid >> 3) + 32 * it;
      const int n = n0 + nl;
      if (kp >= K) continue;               // (the drain skips these image rows too)
      uint4 w = make_uint4(0x77777777u, 0x77777777u, 0x77777777u, 0x77777777u);   // code 7 = 0.0: rows past N fill pad columns
      float a = 0.f;
      if (n < N) {
        w = *reinterpret_cast<const uint4*>(packed + (long)n * (K >> 1) + (kp >> 1));
        a = absmax[(long)n * (K >> 6) + (kp >> 6)];
      }
      const unsigned wd[4] = {w.x, w.y, w.z, w.w};
      unsigned short* col = reinterpret_cast<unsigned short*>(tile) + (32 * p) * kT_N + ((nl + 8 * p) & (kT_N - 1));
#pragma unroll
      for (int b = 0; b < 16; ++b) {       // byte b: codes 2 b (high nibble) and 2 b + 1
        const nf4_f2 t = tab[(wd[b >> 2] >> (8 * (b & 3))) & 255u];
        // the product rounded to fp32 FIRST, then to f16 (a scalar (f16)(x * a) compiles to one mixed-precision multiply with a
        // single rounding: one f16 ulp off wherever the fp32 product lands on an f16 tie)
        const unsigned pk = pack_f16x2(__fmul_rn(t.x, a), __fmul_rn(t.y, a));
        col[(2 * b) * kT_N] = (unsigned short)(pk & 0xffffu);
        col[(2 * b + 1) * kT_N] = (unsigned short)(pk >> 16);
      }
    }
  }
  __syncthreads();
  const int ch = tid & 7;
  const int nc = n0 + 8 * ch;              // first stored row of this lane's chunk
  if (nc >= Np) return;
  int m[8];
  bool whole = true;                       // one 16-B store per k row
  if (row_map) {
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = nc + j < N ? row_map[nc + j] : -1;
#pragma unroll
    for (int j = 0; j < 8; ++j) whole = whole && m[j] == m[0] + j;
    whole = whole && m[0] >= 0 && (m[0] & 7) == 0;
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) m[j] = nc + j;
  }
#pragma unroll
  for (int it = 0; it < 8; ++it) {         // image rows 32 it + tid / 8: piece it, rotation 8 it
    const int kl = 32 * it + (tid >> 3);
    const int k = k0 + kl;
    if (k >= K) break;
    const f16x8 v = *reinterpret_cast<const f16x8*>(tile + kl * kT_N + ((8 * ch + 8 * it) & (kT_N - 1)));
    f16_t* dst = out + (long)k * ldo;
    if (whole) {
      *reinterpret_cast<f16x8*>(dst + m[0]) = v;
    } else {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        if (nc + j < N) dst[m[j]] = v[j];
        else if (nc + j < Np) dst[nc + j] = (f16_t)0.f;
      }
    }
  }
}

struct Nf4Args {
  const bf16_t* A; long lda;
  const unsigned char* Wq; const float* absmax;
  void* C; long ldc;
  const float* bias;
  const void* resid; long ldr;
  const int* row_map;
  int M, N, K, act, out_f32;
};

// Unmerged LoRA adapters of a fused weight (serving adapters fitted on the NF4 base): t = x . A_cat^T as f16 [M][ldt], 8 rank
// values per row segment; B f16 [N][8], each stored row's own coefficients; stored row n belongs to segment (n / seg_rows) % nseg
// (q | k | v: 3 segments of H rows; [gate x16 | up x16]: 2 of 16; o / down: 1). An unadapted segment has zero coefficients.
struct Nf4LoraArgs : Nf4Args {
  const bf16_t* t; long ldt;
  const bf16_t* B;
  int nseg, seg_rows;
  float scale;
};

// Activation 16-B fragments per 64-block per tile row of 16: two k-steps (quant_batch blocks per batch of loads).
// LORA: the rank update s * sum_j t[m][8 seg + j] * B[n][j] joins the reduced sums before bias, activation, SwiGLU and residual,
// as ONE MFMA per 16 x 16 tile (the trick of lora_qkv_rope_fwd_kernel): the weight operand of lane (fr, fh) holds row fr's 8
// coefficients where fh is the row tile's segment and zeros elsewhere, the activation operand t[m][8 fh .. 8 fh + 7].
template <int MT, int NT, bool SWIGLU, int KW, bool LORA = false>
__global__ __launch_bounds__(64 * KW) void gemm_nf4_kernel(std::conditional_t<LORA, Nf4LoraArgs, Nf4Args> p) {
  using E = h16<true>;
  static_assert(!SWIGLU || (NT % 2) == 0, "SwiGLU pairs a gate tile with an up tile");
  constexpr int U = quant_batch<MT>();
  __shared__ nf4_f2 lut[256];                 // byte -> {NF4[byte >> 4], NF4[byte & 15]} (element order in memory: even k first)
  __shared__ float red[KW][MT][64][4];
  for (int b = threadIdx.x; b < 256; b += 64 * KW) lut[b] = nf4_f2{kNF4[b >> 4], kNF4[b & 15]};
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int fr = lane & 15, fh = lane >> 4;
  const int n0 = blockIdx.x * 16 * NT;
  const int kb = p.K >> 6;                     // 64-blocks per row
  const int c_lo = (int)((long)wave * kb / KW), c_hi = (int)((long)(wave + 1) * kb / KW);
  const bf16_t* xrow[MT];
#pragma unroll
  for (int mt = 0; mt < MT; ++mt) xrow[mt] = p.A + (long)min(mt * 16 + fr, p.M - 1) * p.lda + 16 * fh;
  const unsigned char* wrow[NT];
  const float* arow[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const long n = min(n0 + t * 16 + fr, p.N - 1);
    wrow[t] = p.Wq + n * (p.K >> 1) + 8 * fh;
    arow[t] = p.absmax + n * kb;
  }
  // (LORA) both operands of the rank update, requested ahead of the K loop; every wave loads (clamped rows), waves < MT use them
  uint4 lb[LORA ? NT : 1], lt = uint4{0u, 0u, 0u, 0u};
  if constexpr (LORA) {
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const int seg = ((n0 + t * 16) / p.seg_rows) % p.nseg;
      lb[t] = uint4{0u, 0u, 0u, 0u};
      if (fh == seg) lb[t] = *reinterpret_cast<const uint4*>(p.B + (long)min(n0 + t * 16 + fr, p.N - 1) * 8);
    }
    if (fh < p.nseg) lt = *reinterpret_cast<const uint4*>(p.t + (long)min(wave * 16 + fr, p.M - 1) * p.ldt + 8 * fh);
  }
  f32x4 acc[NT][MT];
#pragma unroll
  for (int t = 0; t < NT; ++t)
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) acc[t][mt] = f32x4{0.f, 0.f, 0.f, 0.f};
  uint2 wv[2][NT][U];
  float av[2][NT][U];
  uint4 xv[2][MT][U][2];
  auto load = [&](int set, int c) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int cc = min(c + u, c_hi - 1);     // tail: re-read, skipped at the MFMA
#pragma unroll
      for (int t = 0; t < NT; ++t) {
        wv[set][t][u] = *reinterpret_cast<const uint2*>(wrow[t] + 32L * cc);
        av[set][t][u] = arow[t][cc];
      }
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        xv[set][mt][u][0] = *reinterpret_cast<const uint4*>(xrow[mt] + 64L * cc);
        xv[set][mt][u][1] = *reinterpret_cast<const uint4*>(xrow[mt] + 64L * cc + 8);
      }
    }
  };
  // four packed bytes (8 codes) -> one f16x8 fragment
  auto dq8 = [&](unsigned w, float a) {
    unsigned r[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const nf4_f2 e = lut[(w >> (8 * i)) & 0xffu] * nf4_f2{a, a};
      r[i] = pack_f16x2(e.x, e.y);
    }
    return __builtin_bit_cast(bf16x8, uint4{r[0], r[1], r[2], r[3]});
  };
  auto compute = [&](int set, int c) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (c + u < c_hi) {
#pragma unroll
        for (int t = 0; t < NT; ++t) {
          const bf16x8 w0 = dq8(wv[set][t][u].x, av[set][t][u]);
          const bf16x8 w1 = dq8(wv[set][t][u].y, av[set][t][u]);
#pragma unroll
          for (int mt = 0; mt < MT; ++mt) {
            acc[t][mt] = E::mfma16(w0, __builtin_bit_cast(bf16x8, xv[set][mt][u][0]), acc[t][mt]);
            acc[t][mt] = E::mfma16(w1, __builtin_bit_cast(bf16x8, xv[set][mt][u][1]), acc[t][mt]);
          }
        }
      }
    }
  };
  __syncthreads();   // lut
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
  // the KW partial tiles meet in LDS, in wave order; wave w then owns activation tile w (lane: D[n = 4 fh + r][m = 16 w + fr])
  float o[NT][4];
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      float v[4] = {acc[t][mt][0], acc[t][mt][1], acc[t][mt][2], acc[t][mt][3]};
      store4(&red[wave][mt][lane][0], v);
    }
    __syncthreads();
    if (wave < MT) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float sum = 0.f;
#pragma unroll
        for (int w4 = 0; w4 < KW; ++w4) sum += red[w4][wave][lane][r];
        o[t][r] = sum;
      }
      if constexpr (LORA) {
        const f32x4 d = E::mfma16(__builtin_bit_cast(bf16x8, lb[t]), __builtin_bit_cast(bf16x8, lt), f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
        for (int r = 0; r < 4; ++r) o[t][r] += p.scale * d[r];
      }
    }
    if (t + 1 < NT) __syncthreads();
  }
  if (wave >= MT) return;
  const int m = wave * 16 + fr;
  if (m >= p.M) return;
  long orow = m;
  if (p.row_map) {
    orow = p.row_map[m];
    if (orow < 0) return;
  }
  const int n_total_out = SWIGLU ? (p.N >> 1) : p.N;
  constexpr int NOUT = SWIGLU ? NT / 2 : NT;
#pragma unroll
  for (int j = 0; j < NOUT; ++j) {
    float val[4];
    const int nb = (SWIGLU ? (n0 >> 1) : n0) + 16 * j + 4 * fh;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if constexpr (SWIGLU) {
        const int ng = n0 + 32 * j + 4 * fh + r, nu = ng + 16;
        const float g = o[2 * j][r] + (p.bias ? p.bias[min(ng, p.N - 1)] : 0.f);
        const float u = o[2 * j + 1][r] + (p.bias ? p.bias[min(nu, p.N - 1)] : 0.f);
        val[r] = g * __builtin_amdgcn_rcpf(1.0f + __expf(-g)) * u;
      } else {
        val[r] = apply_act(o[j][r] + (p.bias ? p.bias[min(nb + r, p.N - 1)] : 0.f), p.act);
      }
    }
    if (nb >= n_total_out) continue;
    if (p.out_f32) {
      float* c = reinterpret_cast<float*>(p.C) + orow * p.ldc + nb;
      const float* rs = p.resid ? reinterpret_cast<const float*>(p.resid) + orow * p.ldr + nb : nullptr;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (nb + r < n_total_out) c[r] = val[r] + (rs ? rs[r] : 0.f);
    } else {
      f16_t* c = reinterpret_cast<f16_t*>(p.C) + orow * p.ldc + nb;
      const f16_t* rs = p.resid ? reinterpret_cast<const f16_t*>(p.resid) + orow * p.ldr + nb : nullptr;
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (nb + r < n_total_out) c[r] = (f16_t)(val[r] + (rs ? (float)rs[r] : 0.f));
    }
  }
}

template <int MT, bool LORA, typename Args>
void launch_nf4(const Args& p, int swiglu, hipStream_t s) {
  const int nt = quant_raster_nt(p.N, MT, swiglu);
  const dim3 g = quant_grid(p.N, nt), b(64 * kQuantWaves);
  if (swiglu) hipLaunchKernelGGL((gemm_nf4_kernel<MT, 2, true, kQuantWaves, LORA>), g, b, 0, s, p);
  else if (nt == 2) hipLaunchKernelGGL((gemm_nf4_kernel<MT, 2, false, kQuantWaves, LORA>), g, b, 0, s, p);
  else hipLaunchKernelGGL((gemm_nf4_kernel<MT, 1, false, kQuantWaves, LORA>), g, b, 0, s, p);
}

// The host-side rules the entry points below share, one function each (haff_aligned: on that many bytes, or null).
// The stored rows of a weight: whole 64-blocks, both tables present, the absmax on a float, the codes on the kernel's widest access to
// them: 4 bytes in the quantiser and the row-major dequantisers (a thread's word of 8 codes), 8 in the products, 16 transposed
bool nf4_rows_bad(const void* packed, unsigned packed_align, const float* absmax, int N, int K) {
  return N <= 0 || K <= 0 || (K & 63) || !packed || !absmax || !haff_aligned(packed, packed_align) || !haff_aligned(absmax, 4);
}
// f16 rows read or written 8 elements at a time: present, on 16 bytes, a stride of whole chunks that holds `cols` elements
bool nf4_f16_rows_bad(const void* p, long ld, long cols) { return !p || !haff_aligned(p) || (ld & 7) || ld < cols; }

// the refusals of both products (0: go on); -2 comes right after the zero dimensions, ahead of every other -1 rule
int nf4_gemm_args_bad(const void* A, long lda, const void* Wq, const float* absmax, const void* C, const void* resid, int M, int N, int K,
                      int swiglu) {
  if (M <= 0 || N <= 0 || K <= 0) return HAFF_ERR_BAD_ARG;
  if (M > 64) return HAFF_ERR_UNSUPPORTED;   // decode-sized products only: prefill dequantises and runs haff_gemm_f16
  if (nf4_rows_bad(Wq, 8, absmax, N, K) || nf4_f16_rows_bad(A, lda, K) || !C) return HAFF_ERR_BAD_ARG;
  if (swiglu && ((N & 31) || resid)) return HAFF_ERR_BAD_ARG;
  return 0;
}

// ... and of the adapters' layout, shared by both LoRA entry points
bool nf4_lora_layout_bad(const void* B, int nseg, int seg_rows) {
  return nseg < 1 || nseg > 4 || seg_rows <= 0 || (seg_rows & 15) || !B || !haff_aligned(B);
}

// The argument block of both products, every field BY NAME (Nf4LoraArgs adds its own to it)
void nf4_args(Nf4Args& p, const void* A, long lda, const void* Wq, const float* absmax, void* C, long ldc, const float* bias,
              const void* resid, long ldr, const int* row_map, int M, int N, int K, int act, int out_f32) {
  p.A = reinterpret_cast<const bf16_t*>(A); p.lda = lda;
  p.Wq = reinterpret_cast<const unsigned char*>(Wq); p.absmax = absmax;
  p.C = C; p.ldc = ldc; p.bias = bias; p.resid = resid; p.ldr = ldr; p.row_map = row_map;
  p.M = M; p.N = N; p.K = K; p.act = act; p.out_f32 = out_f32;
}

}  // namespace

extern "C" int haff_nf4_quantize_f16(const void* W, long ldw, int N, int K, int double_quant, const int* row_map, void* packed,
                                     float* absmax, float* offset, void* workspace, long workspace_bytes, void* stream) {
  if (nf4_rows_bad(packed, 4, absmax, N, K) || nf4_f16_rows_bad(W, ldw, K) || (double_quant != 0 && double_quant != 1)) return HAFF_ERR_BAD_ARG;
  if (!offset || !workspace || !haff_aligned(workspace, 4)) return HAFF_ERR_BAD_ARG;
  const long nb = (long)N * (K >> 6);
  if (workspace_bytes < 4 * nb) return HAFF_ERR_BAD_ARG;
  hipStream_t s = haff_stream(stream);
  float* amax_src = reinterpret_cast<float*>(workspace);
  const long thr = (long)N * (K >> 3);
  hipLaunchKernelGGL(nf4_codes_kernel, dim3((unsigned)((thr + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const bf16_t*>(W), ldw, N,
                     K, row_map, reinterpret_cast<unsigned char*>(packed), amax_src);
  hipLaunchKernelGGL(nf4_offset_kernel, dim3(1), dim3(256), 0, s, amax_src, nb, offset);
  hipLaunchKernelGGL(nf4_absmax_kernel, dim3((unsigned)((nb + 255) / 256)), dim3(256), 0, s, amax_src, nb, K >> 6, row_map, double_quant,
                     offset, absmax);
  return haff_check_launch();
}

extern "C" int haff_nf4_dequant_f16(const void* packed, const float* absmax, int N, int K, const int* row_map, void* out, long ldo,
                                    void* stream) {
  if (nf4_rows_bad(packed, 4, absmax, N, K) || nf4_f16_rows_bad(out, ldo, K)) return HAFF_ERR_BAD_ARG;
  const long thr = (long)N * (K >> 3);
  hipLaunchKernelGGL(nf4_dequant_kernel, dim3((unsigned)((thr + 255) / 256)), dim3(256), 0, haff_stream(stream),
                     reinterpret_cast<const unsigned char*>(packed), absmax, N, K, row_map, reinterpret_cast<bf16_t*>(out), ldo);
  return haff_check_launch();
}

extern "C" int haff_nf4_dequant_t_f16(const void* packed, const float* absmax, int N, int K, const int* row_map, void* out_t, long ldo,
                                      void* stream) {
  // unlike the row-major forms: the fill reads 16-byte code chunks (packed on 16 bytes, not 4), an output row holds the stored rows
  // padded to whole 8-column chunks (ldo >= roundup(N, 8), not K), and the row map's alignment is asked for
  if (nf4_rows_bad(packed, 16, absmax, N, K) || nf4_f16_rows_bad(out_t, ldo, (N + 7) & ~7) || !haff_aligned(row_map, 4)) return HAFF_ERR_BAD_ARG;
  hipLaunchKernelGGL(nf4_dequant_t_kernel, dim3((unsigned)((K + kT_K - 1) / kT_K), (unsigned)((N + kT_N - 1) / kT_N)), dim3(256), 0,
                     haff_stream(stream), reinterpret_cast<const unsigned char*>(packed), absmax, N, K, row_map,
                     reinterpret_cast<f16_t*>(out_t), ldo);
  return haff_check_launch();
}

extern "C" int haff_gemm_nf4_f16(const void* A, long lda, const void* Wq, const float* absmax, void* C, long ldc, const float* bias,
                                 const void* resid, long ldr, const int* row_map, int M, int N, int K, int act, int out_f32, int swiglu,
                                 void* stream) {
  if (const int bad = nf4_gemm_args_bad(A, lda, Wq, absmax, C, resid, M, N, K, swiglu)) return bad;
  Nf4Args p;
  nf4_args(p, A, lda, Wq, absmax, C, ldc, bias, resid, ldr, row_map, M, N, K, act, out_f32);
  HAFF_DISPATCH_MT(M, launch_nf4<MT, false>(p, swiglu, haff_stream(stream)));
  return haff_check_launch();
}

extern "C" int haff_gemm_nf4_lora_f16(const void* A, long lda, const void* Wq, const float* absmax, void* C, long ldc, const float* bias,
                                      const void* resid, long ldr, const int* row_map, int M, int N, int K, int act, int out_f32,
                                      int swiglu, const void* t, long ldt, const void* B, int nseg, int seg_rows, float scale,
                                      void* stream) {
  if (const int bad = nf4_gemm_args_bad(A, lda, Wq, absmax, C, resid, M, N, K, swiglu)) return bad;
  if (nf4_lora_layout_bad(B, nseg, seg_rows) || nf4_f16_rows_bad(t, ldt, 8 * nseg)) return HAFF_ERR_BAD_ARG;
  Nf4LoraArgs p;
  nf4_args(p, A, lda, Wq, absmax, C, ldc, bias, resid, ldr, row_map, M, N, K, act, out_f32);
  p.t = reinterpret_cast<const bf16_t*>(t); p.ldt = ldt; p.B = reinterpret_cast<const bf16_t*>(B);
  p.nseg = nseg; p.seg_rows = seg_rows; p.scale = scale;
  HAFF_DISPATCH_MT(M, launch_nf4<MT, true>(p, swiglu, haff_stream(stream)));
  return haff_check_launch();
}

extern "C" int haff_nf4_dequant_lora_f16(const void* packed, const float* absmax, int N, int K, const int* row_map, void* out, long ldo,
                                         const void* A_cat, long lda, const void* B, int nseg, int seg_rows, float scale,
                                         void* stream) {
  if (nf4_rows_bad(packed, 4, absmax, N, K) || nf4_f16_rows_bad(out, ldo, K)) return HAFF_ERR_BAD_ARG;
  if (nf4_lora_layout_bad(B, nseg, seg_rows) || nf4_f16_rows_bad(A_cat, lda, K)) return HAFF_ERR_BAD_ARG;
  const long thr = (long)((N + 7) >> 3) * (K >> 3);
  hipLaunchKernelGGL(nf4_dequant_lora_kernel, dim3((unsigned)((thr + 255) / 256)), dim3(256), 0, haff_stream(stream),
                     reinterpret_cast<const unsigned char*>(packed), absmax, N, K, row_map, reinterpret_cast<f16_t*>(out), ldo,
                     reinterpret_cast<const f16_t*>(A_cat), lda, reinterpret_cast<const f16_t*>(B), nseg, seg_rows, scale);
  return haff_check_launch();
}
