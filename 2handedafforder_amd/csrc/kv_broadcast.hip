// Shared-prefix K/V broadcast (LisaMI355.evaluate(offset=), lisa.py): several prompt rows of one frame share the first P cached
// positions. The prefix is prefilled once per frame into an [F][tmax_src][H] cache; this kernel copies positions 0 .. P-1 of both K and V
// of frame frame_of[b] into row b of the ordinary [B][tmax_dst][H] cache, one launch per layer.
//
// Pure data movement. Positions are H * elem bytes apart in both caches, so a row's prefix is ONE contiguous run of P * H * elem bytes
// (a multiple of 16): the kernel sees 16-byte units only and never the element type. No LDS; plain dwordx4 loads and stores — the
// loads so that the XCD's L2 / the Infinity Cache serve the re-reads of a frame's block by the other rows of that frame, the stores
// because the tail prefill's attention reads the destination next and the whole row set (150 MB per tensor at 7B, 64 rows) fits the
// 256 MiB Infinity Cache.
//
// Grid: sized by bytes, one 16 KiB chunk of K and of V per 256-thread workgroup (4 units per lane and tensor, all 8 loads issued before
// the first store). Linear workgroup id = chunk * B + row: consecutive workgroups take the SAME chunk of consecutive rows, so every
// consumer of a frame's chunk is in flight together and the caches can serve the re-reads. The values are held in plain vector registers
// (ext_vector_type: conditionally filled uint4 arrays end up in scratch and LDS). Bound: the HBM write of 2 * B * P * H * elem bytes.
#include "haff_common.h"

#include <limits.h>

namespace {

constexpr int kThreads = 256;
constexpr int kUnroll = 4;                                // 16-byte units per lane and tensor
constexpr long kChunkUnits = (long)kThreads * kUnroll;    // 16 KiB per tensor per workgroup
static_assert(kUnroll == 4, "the whole-chunk arm of the kernel is written out for four units");
typedef unsigned unit_t __attribute__((ext_vector_type(4)));   // one 16-byte unit: a dwordx4 load / store, a plain register value

// units = P * H * elem / 16 per row; strides in 16-byte units. frame_of[b] is read once per workgroup (a uniform load); an entry
// outside [0, F) is not dereferenced: that row is left untouched (the host validates the map, prompt_groups.check_offset).
__global__ __launch_bounds__(kThreads) void kv_prefix_broadcast_kernel(const unit_t* __restrict__ k_src, const unit_t* __restrict__ v_src,
                                                                       long src_row_units, unit_t* __restrict__ k_dst,
                                                                       unit_t* __restrict__ v_dst, long dst_row_units,
                                                                       const int* __restrict__ frame_of, int B, int F, long units) {
  const int b = blockIdx.x % B;
  const long chunk = blockIdx.x / B;
  const int f = frame_of[b];
  if ((unsigned)f >= (unsigned)F) return;
  const long base = chunk * kChunkUnits + threadIdx.x;
  const unit_t* ks = k_src + (long)f * src_row_units;
  const unit_t* vs = v_src + (long)f * src_row_units;
  unit_t* kd = k_dst + (long)b * dst_row_units;
  unit_t* vd = v_dst + (long)b * dst_row_units;
  if (base + (long)(kUnroll - 1) * kThreads < units) {
    // a whole chunk (all but the last of a row): every load in flight before the first store, the values in registers
    const unit_t k0 = ks[base], k1 = ks[base + kThreads], k2 = ks[base + 2 * kThreads], k3 = ks[base + 3 * kThreads];
    const unit_t v0 = vs[base], v1 = vs[base + kThreads], v2 = vs[base + 2 * kThreads], v3 = vs[base + 3 * kThreads];
    kd[base] = k0; kd[base + kThreads] = k1; kd[base + 2 * kThreads] = k2; kd[base + 3 * kThreads] = k3;
    vd[base] = v0; vd[base + kThreads] = v1; vd[base + 2 * kThreads] = v2; vd[base + 3 * kThreads] = v3;
    return;
  }
  for (long i = base; i < units; i += kThreads) {   // the row's last, partly filled chunk
    const unit_t k = ks[i], v = vs[i];
    kd[i] = k;
    vd[i] = v;
  }
}

}  // namespace

extern "C" int haff_kv_prefix_broadcast(const void* k_src, const void* v_src, long src_row_stride, void* k_dst, void* v_dst,
                                        long dst_row_stride, const int* frame_of, int B, int F, int P, int H, int dtype, void* stream) {
  if (!k_src || !v_src || !k_dst || !v_dst || !frame_of || B < 1 || F < 1 || P < 1 || H < 1) return HAFF_ERR_BAD_ARG;
  long elem = 0;                                          // bytes per element: the kernel never sees the type
  HAFF_DISPATCH(dtype, elem = sizeof(T));
  const long row_bytes = (long)H * elem;
  const long run = (long)P * H;                           // elements of one row's prefix
  if (row_bytes % 16 || src_row_stride < run || dst_row_stride < run || (src_row_stride * elem) % 16 || (dst_row_stride * elem) % 16)
    return HAFF_ERR_BAD_ARG;
  if (!haff_aligned(k_src) || !haff_aligned(v_src) || !haff_aligned(k_dst) || !haff_aligned(v_dst) || !haff_aligned(frame_of, 4))
    return HAFF_ERR_BAD_ARG;
  const long units = run * elem / 16;
  const long chunks = (units + kChunkUnits - 1) / kChunkUnits;
  if (chunks * B > INT_MAX) return HAFF_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(kv_prefix_broadcast_kernel, dim3((unsigned)(chunks * B)), dim3(kThreads), 0, haff_stream(stream),
                     (const unit_t*)k_src, (const unit_t*)v_src, src_row_stride * elem / 16, (unit_t*)k_dst, (unit_t*)v_dst,
                     dst_row_stride * elem / 16, frame_of, B, F, units);
  return haff_check_launch();
}
