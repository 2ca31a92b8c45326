// What the two weight-streaming products on quantised weights share (gemm_nf4_kernel in gemm_nf4.hip, gemm_i8_skinny_kernel in
// gemm_int8.hip): the workgroup's geometry and the host-side choice of the instance. The kernels stay whole in their own files. That
// includes the final store (row map, n_out edge, residual, f16 / fp32), which reads the same in both: called as a shared
// __device__ function, in any form tried, it moved instructions in every instance of both kernels, so each keeps its copy.
#pragma once
#include "haff_common.h"

// One workgroup = 16 * NT weight rows, 8 waves splitting K into contiguous ranges of 64-deep blocks
constexpr int kQuantWaves = 8;

// Blocks per batch of loads (two register sets), by the activation row tiles of 16 a lane feeds
template <int MT> constexpr int quant_batch() { return MT == 1 ? 4 : (MT == 2 ? 2 : 1); }

// host side, the raster rule: 16 weight rows per workgroup (NT = 1) while the wider form would leave fewer than 192 workgroups; 32
// (NT = 2) otherwise, and always under SwiGLU, which pairs a gate tile with an up tile
static inline int quant_raster_nt(int N, int MT, int swiglu) {
  const int tiles = (N + 15) / 16;
  return swiglu || (MT >= 2 && tiles / 2 >= 192) ? 2 : 1;
}
static inline dim3 quant_grid(int N, int nt) { return dim3(((N + 15) / 16 + nt - 1) / nt); }

// host side: the statement with the compile-time constant MT = the activation row tiles of 16 that serve M <= 64 rows (1, 2 or 4)
#define HAFF_DISPATCH_MT(M, ...) \
  do { \
    if ((M) <= 16) { constexpr int MT = 1; __VA_ARGS__; } \
    else if ((M) <= 32) { constexpr int MT = 2; __VA_ARGS__; } \
    else { constexpr int MT = 4; __VA_ARGS__; } \
  } while (0)
