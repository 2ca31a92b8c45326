// Shared device helpers for the 2HandedAfforder MI355X (gfx950 / CDNA4) hot path.
// Wave = 64 lanes everywhere; bf16 is carried as raw 16-bit payloads (unsigned short).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
// the public declarations (and the return codes): every extern "C" definition in csrc/ is compiled against its declaration
#include "haff_hip.h"
#include <cstddef>

// A kernel-side struct K mirrors a public descriptor P of haff_hip.h (the kernels keep their own names: a rename would change the
// mangled kernel names). HAFF_SAME_SIZE once per pair, HAFF_SAME_FIELD for every field.
#define HAFF_SAME_SIZE(K, P) static_assert(sizeof(K) == sizeof(P), #K " and " #P " differ in size")
#define HAFF_SAME_FIELD(K, kf, P, pf) \
  static_assert(offsetof(K, kf) == offsetof(P, pf) && sizeof(K::kf) == sizeof(P::pf), #K "::" #kf " is not " #P "::" #pf)

typedef unsigned short bf16_t;
typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) short bf16x4;
typedef __attribute__((ext_vector_type(2))) short bf16x2;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

#define HAFF_WAVE 64

// activation codes shared by the GEMM epilogues (see include/haff_hip.h)
#define HAFF_ACT_NONE 0
#define HAFF_ACT_GELU 1        // exact erf GELU (SAM encoder MLP, upscaler)
#define HAFF_ACT_QUICK_GELU 2  // x*sigmoid(1.702x) (CLIP)
#define HAFF_ACT_RELU 3        // SAM decoder MLPs
#define HAFF_ACT_SILU 4

// a * b + c * d with an error of about two fp32 ulps of the RESULT (Kahan's algorithm; the rotate-half RoPE of the cache kernels):
// the plain form rounds both products at the size of the operands, and where they cancel below 2^-12 of them that error exceeds
// an f16 ulp of the result (1.51 storage ulps from the float64 rotation:
// tests/test_attn_edge_kernels_gpu.py::test_decode_rope_appended_k_row). Here the rounding error e of c * d is exact (one fma)
// and is added back after the fma that sums the two products: two roundings, the fma's and the last add's, both at the size of
// the result.
__device__ __forceinline__ float haff_sum_of_products(float a, float b, float c, float d) {
  const float p = c * d;
  const float e = __builtin_fmaf(c, d, -p);
  return __builtin_fmaf(a, b, p) + e;
}

__device__ __forceinline__ float bf16_to_f32(bf16_t v) {
  return __uint_as_float(((unsigned)v) << 16);
}
// round-to-nearest-even; a plain cast keeps NaN a NaN (v_cvt_pk_bf16_f32 on gfx950)
__device__ __forceinline__ bf16_t f32_to_bf16(float f) {
  __bf16 h = (__bf16)f;
  return __builtin_bit_cast(bf16_t, h);
}
// two floats -> one dword of two bf16 with ONE v_cvt_pk_bf16_f32 (converting them separately and or-ing the halves
// costs 3-4 VALU ops per pair: measured as a third of the attention kernels' VALU work)
typedef float haff_f32x2 __attribute__((ext_vector_type(2)));
typedef __bf16 haff_bf16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ unsigned pack_bf16x2(float lo, float hi) {
  const haff_f32x2 f = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f, haff_bf16x2));
}

// fp16 (IEEE binary16) rows: a C++ type of their own (bf16_t is unsigned short), so elem<>, load8 / store8 tell them apart.
// f32 -> f16 is the IEEE conversion: round to nearest even, overflow gives +-inf (never a saturated value).
typedef _Float16 f16_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8;
typedef __attribute__((ext_vector_type(2))) _Float16 haff_f16x2;
__device__ __forceinline__ float f16_to_f32(unsigned short v) { return (float)__builtin_bit_cast(_Float16, v); }
__device__ __forceinline__ unsigned short f32_to_f16(float f) { return __builtin_bit_cast(unsigned short, (_Float16)f); }
__device__ __forceinline__ unsigned pack_f16x2(float lo, float hi) {
  const haff_f32x2 f = {lo, hi};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(f, haff_f16x2));
}

// The 16-bit operand format of the MFMA kernels as a compile-time parameter (one kernel, two instances): operands travel as raw
// 16-bit payloads through HBM, LDS and registers either way; h16<F16> supplies the conversions and the MFMA forms.
// lo / hi: the element in the low / high half of a dword.
template <bool F16> struct h16;
template <> struct h16<false> {
  static __device__ __forceinline__ float lo(unsigned w) { return __uint_as_float(w << 16); }
  static __device__ __forceinline__ float hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }
  static __device__ __forceinline__ float to_f32(unsigned short v) { return bf16_to_f32(v); }
  static __device__ __forceinline__ unsigned short from_f32(float f) { return f32_to_bf16(f); }
  static __device__ __forceinline__ unsigned pack2(float lo, float hi) { return pack_bf16x2(lo, hi); }
  static __device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
  static __device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, c, 0, 0, 0);
  }
};
template <> struct h16<true> {
  static __device__ __forceinline__ float lo(unsigned w) { return f16_to_f32((unsigned short)(w & 0xffffu)); }
  static __device__ __forceinline__ float hi(unsigned w) { return f16_to_f32((unsigned short)(w >> 16)); }
  static __device__ __forceinline__ float to_f32(unsigned short v) { return f16_to_f32(v); }
  static __device__ __forceinline__ unsigned short from_f32(float f) { return f32_to_f16(f); }
  static __device__ __forceinline__ unsigned pack2(float lo, float hi) { return pack_f16x2(lo, hi); }
  static __device__ __forceinline__ f32x4 mfma16(bf16x8 a, bf16x8 b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
  static __device__ __forceinline__ f32x16 mfma32(bf16x8 a, bf16x8 b, f32x16 c) {
    return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8, a), __builtin_bit_cast(f16x8, b), c, 0, 0, 0);
  }
};

template <typename T> struct elem;
template <> struct elem<float> {
  static __device__ __forceinline__ float ld(const float* p) { return *p; }
  static __device__ __forceinline__ void st(float* p, float v) { *p = v; }
};
template <> struct elem<bf16_t> {
  static __device__ __forceinline__ float ld(const bf16_t* p) { return bf16_to_f32(*p); }
  static __device__ __forceinline__ void st(bf16_t* p, float v) { *p = f32_to_bf16(v); }
};
template <> struct elem<f16_t> {
  static __device__ __forceinline__ float ld(const f16_t* p) { return (float)*p; }
  static __device__ __forceinline__ void st(f16_t* p, float v) { *p = (f16_t)v; }
};

// 8-element vector load/store (16 B for bf16, 32 B for f32) into fp32 registers
__device__ __forceinline__ void load8(const bf16_t* p, float (&v)[8]) {
  uint4 r = *reinterpret_cast<const uint4*>(p);
  unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = __uint_as_float(w[i] << 16);
    v[2 * i + 1] = __uint_as_float(w[i] & 0xffff0000u);
  }
}
__device__ __forceinline__ void load8(const float* p, float (&v)[8]) {
  float4 a = *reinterpret_cast<const float4*>(p);
  float4 b = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
  v[4] = b.x; v[5] = b.y; v[6] = b.z; v[7] = b.w;
}
__device__ __forceinline__ void store8(bf16_t* p, const float (&v)[8]) {
  uint4 r;
  r.x = pack_bf16x2(v[0], v[1]);
  r.y = pack_bf16x2(v[2], v[3]);
  r.z = pack_bf16x2(v[4], v[5]);
  r.w = pack_bf16x2(v[6], v[7]);
  *reinterpret_cast<uint4*>(p) = r;
}
__device__ __forceinline__ void store8(float* p, const float (&v)[8]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
__device__ __forceinline__ void load4(const bf16_t* p, float (&v)[4]) {
  uint2 r = *reinterpret_cast<const uint2*>(p);
  v[0] = __uint_as_float(r.x << 16); v[1] = __uint_as_float(r.x & 0xffff0000u);
  v[2] = __uint_as_float(r.y << 16); v[3] = __uint_as_float(r.y & 0xffff0000u);
}
__device__ __forceinline__ void load4(const float* p, float (&v)[4]) {
  float4 a = *reinterpret_cast<const float4*>(p);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
}
__device__ __forceinline__ void store4(bf16_t* p, const float (&v)[4]) {
  uint2 r;
  r.x = pack_bf16x2(v[0], v[1]);
  r.y = pack_bf16x2(v[2], v[3]);
  *reinterpret_cast<uint2*>(p) = r;
}
__device__ __forceinline__ void load8(const f16_t* p, float (&v)[8]) {
  uint4 r = *reinterpret_cast<const uint4*>(p);
  unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    v[2 * i] = h16<true>::lo(w[i]);
    v[2 * i + 1] = h16<true>::hi(w[i]);
  }
}
__device__ __forceinline__ void store8(f16_t* p, const float (&v)[8]) {
  uint4 r;
  r.x = pack_f16x2(v[0], v[1]);
  r.y = pack_f16x2(v[2], v[3]);
  r.z = pack_f16x2(v[4], v[5]);
  r.w = pack_f16x2(v[6], v[7]);
  *reinterpret_cast<uint4*>(p) = r;
}
__device__ __forceinline__ void load4(const f16_t* p, float (&v)[4]) {
  uint2 r = *reinterpret_cast<const uint2*>(p);
  v[0] = h16<true>::lo(r.x); v[1] = h16<true>::hi(r.x);
  v[2] = h16<true>::lo(r.y); v[3] = h16<true>::hi(r.y);
}
__device__ __forceinline__ void store4(f16_t* p, const float (&v)[4]) {
  uint2 r;
  r.x = pack_f16x2(v[0], v[1]);
  r.y = pack_f16x2(v[2], v[3]);
  *reinterpret_cast<uint2*>(p) = r;
}
__device__ __forceinline__ void store4(float* p, const float (&v)[4]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
}

// 16-bit rows carried as raw payloads (const bf16_t*) by the kernels templated on the operand format (h16<F16>)
template <bool F16> __device__ __forceinline__ void load8h(const bf16_t* p, float (&v)[8]) {
  if constexpr (F16) load8(reinterpret_cast<const f16_t*>(p), v); else load8(p, v);
}
template <bool F16> __device__ __forceinline__ void store8h(bf16_t* p, const float (&v)[8]) {
  if constexpr (F16) store8(reinterpret_cast<f16_t*>(p), v); else store8(p, v);
}
template <bool F16> __device__ __forceinline__ void store4h(bf16_t* p, const float (&v)[4]) {
  if constexpr (F16) store4(reinterpret_cast<f16_t*>(p), v); else store4(p, v);
}

__device__ __forceinline__ float apply_act(float x, int act) {
  switch (act) {
    case HAFF_ACT_GELU: return 0.5f * x * (1.0f + erff(x * 0.70710678118654752440f));
    case HAFF_ACT_QUICK_GELU: return x / (1.0f + __expf(-1.702f * x));
    case HAFF_ACT_RELU: return fmaxf(x, 0.0f);
    case HAFF_ACT_SILU: return x / (1.0f + __expf(-x));
    default: return x;
  }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

// OpenCV's borderInterpolate for BORDER_REFLECT_101 (gfedcb|abcdefgh|gfedcba), any overshoot
__device__ __forceinline__ int reflect101(int p, int len) {
  if (len == 1) return 0;
  while ((unsigned)p >= (unsigned)len) p = p < 0 ? -p : 2 * len - 2 - p;
  return p;
}

static inline int haff_check_launch() {
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? HAFF_OK : HAFF_ERR_LAUNCH;
}
static inline hipStream_t haff_stream(void* stream) { return reinterpret_cast<hipStream_t>(stream); }
// host side: blocks of `block` threads that cover `total` items, at least 1 and at most `cap` (the grid-stride kernels take the rest)
static inline int haff_grid(long total, int block, long cap) {
  const long g = (total + block - 1) / block;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}
// host side, storage-type dispatch: runs the statement with T = the element type of dtype code 0 (bf16), 1 (f32) or 3 (f16) and
// RETURNS HAFF_ERR_BAD_ARG from the calling function for any other code, before a launch (code 2 is the norms' mixed form, a
// special case of norm.hip). HAFF_DISPATCH_16 serves the 16-bit-only vector paths: codes 0 and 3.
#define HAFF_DISPATCH_CASE_(code, type, ...) case code: { using T = type; __VA_ARGS__; } break;
#define HAFF_DISPATCH(dtype, ...) \
  do { switch (dtype) { \
    HAFF_DISPATCH_CASE_(0, bf16_t, __VA_ARGS__) \
    HAFF_DISPATCH_CASE_(1, float, __VA_ARGS__) \
    HAFF_DISPATCH_CASE_(3, f16_t, __VA_ARGS__) \
    default: return HAFF_ERR_BAD_ARG; \
  } } while (0)
#define HAFF_DISPATCH_16(dtype, ...) \
  do { switch (dtype) { \
    HAFF_DISPATCH_CASE_(0, bf16_t, __VA_ARGS__) \
    HAFF_DISPATCH_CASE_(3, f16_t, __VA_ARGS__) \
    default: return HAFF_ERR_BAD_ARG; \
  } } while (0)
// the statement with the compile-time constant NAME = (cond), true first
#define HAFF_DISPATCH_BOOL(cond, NAME, ...) \
  do { if (cond) { constexpr bool NAME = true; __VA_ARGS__; } else { constexpr bool NAME = false; __VA_ARGS__; } } while (0)
// the statement with T = the output type of the TN products' reduce kernels: float when out_f32 is set, else f16_t (F16) or bf16_t
#define HAFF_DISPATCH_OUT16(out_f32, F16, ...) \
  do { if (out_f32) { using T = float; __VA_ARGS__; } else if (F16) { using T = f16_t; __VA_ARGS__; } else { using T = bf16_t; __VA_ARGS__; } } while (0)
// host side: p sits on a `bytes` boundary (a power of two; 16 = one dwordx4 access). A null pointer passes.
static inline bool haff_aligned(const void* p, unsigned bytes = 16) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; }
// host side: the (batch, head, token) strides of q / k / v are multiples of in_mask + 1 elements, those of the output of out_mask + 1
// (16-bit attention: 7 / 3, whole 16-byte input chunks and 8-byte output chunks; f32: 3 / 3)
static inline bool haff_strides_ok(long q_sb, long q_sh, long q_st, long k_sb, long k_sh, long k_st, long v_sb, long v_sh, long v_st,
                                   long o_sb, long o_sh, long o_st, long in_mask, long out_mask) {
  return !(((q_sb | q_sh | q_st | k_sb | k_sh | k_st | v_sb | v_sh | v_st) & in_mask) || ((o_sb | o_sh | o_st) & out_mask));
}
