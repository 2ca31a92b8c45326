// Device-side ground-truth masks of the fine-tune loader: cv2.drawContours(mask, [contour], -1, 1, FILLED) per contour
// (utils/aff_dataset.py:340-346) for a whole batch of planes in one call, bit for bit with cvlite.draw_contours_filled.
//
//   haff_fill_contours_u8 : zero the planes (hipMemsetAsync, part of the call), then two kernels that only ever store the value 1,
//                           so neither their order nor races between polygons change a byte:
//     outline_kernel : one wave per polygon edge (the closing edge last -> first included). cvlite._line8's Bresenham walk from the
//                      smaller-x end has a closed form: pixel i (0 <= i <= major) has taken floor((2*minor*i + major - 1) / (2*major))
//                      minor-axis steps, so the lanes take pixels i, i + 64, ...; clipped per pixel.
//     fill_kernel    : one wave per (polygon, row). The 16.16 crossings of the row (int64: x0 * 65536 + (y - y0) * dx with
//                      dx = trunc((x1 - x0) * 65536 / (y1 - y0))) are compacted into LDS by ballot in passes of 64 edges; every
//                      crossing finds its rank and its successor in (value, edge index) order by one scan of the list, the even
//                      ranks emit the span [x >> 16, next >> 16] and the wave fills each span with 64 consecutive byte stores per step.
//                      The list is sized by the longest polygon of the launch (12 bytes per vertex of LDS, at most 48 KB), so no
//                      row can overflow it: there is no data-dependent failure on the device.
// Everything a kernel indexes with is checked on the HOST copy of the descriptors before anything is enqueued.
#include <limits.h>

#include "haff_common.h"

#define HAFF_FILL_MAX_VERTS 4096    // vertices per polygon (LDS: 12 bytes each)
#define HAFF_FILL_MAX_COORD 32768   // |x|, |y| < this: (x1 - x0) * 65536 and 2 * minor * i stay far inside int64

namespace {

// polygon that owns vertex v: the last p with off[p] <= v (empty polygons share an offset with their successor and are skipped)
__device__ __forceinline__ int poly_of(const int* off, int n_poly, int v) {
  int lo = 0, hi = n_poly - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (off[mid] <= v) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__global__ __launch_bounds__(256) void outline_kernel(const int* off, const int* plane, const int* pts, int n_poly, int n_pts,
                                                      unsigned char* out, int H, int W) {
  const int lane = threadIdx.x & 63;
  const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  const int n_waves = (int)((gridDim.x * blockDim.x) >> 6);
  for (int v = wave; v < n_pts; v += n_waves) {
    const int p = poly_of(off, n_poly, v);
    const int first = off[p], last = off[p + 1] - 1;
    const int u = v == first ? last : v - 1;                 // the edge runs from the previous vertex (cvlite.fill_poly)
    int x0 = pts[2 * u], y0 = pts[2 * u + 1], x1 = pts[2 * v], y1 = pts[2 * v + 1];
    if (x1 < x0) {                                           // leftToRight: start from the smaller-x end
      int t = x0; x0 = x1; x1 = t;
      t = y0; y0 = y1; y1 = t;
    }
    const int dx = x1 - x0;
    const int sy = y1 >= y0 ? 1 : -1;
    const int dy = y1 >= y0 ? y1 - y0 : y0 - y1;
    const bool steep = dy > dx;
    const int major = steep ? dy : dx, minor = steep ? dx : dy;
    unsigned char* o = out + (long)plane[p] * H * W;
    for (int i = lane; i <= major; i += 64) {
      const int c = major > 0 ? (int)((2LL * minor * i + major - 1) / (2LL * major)) : 0;
      const int x = steep ? x0 + c : x0 + i;
      const int y = steep ? y0 + sy * i : y0 + sy * c;
      if (x >= 0 && x < W && y >= 0 && y < H) o[(long)y * W + x] = 1;
    }
  }
}

// grid (row groups, polygons), one wave per block; dynamic LDS: long long cross[max_verts] | int span[max_verts / 2 + 1][2]
__global__ __launch_bounds__(64) void fill_kernel(const int* off, const int* plane, const int* pts, unsigned char* out, int H, int W,
                                                  int max_verts) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fsm[];
  long long* cross = reinterpret_cast<long long*>(fsm);
  int* span = reinterpret_cast<int*>(fsm + (size_t)max_verts * 8);
  const int lane = threadIdx.x;
  const int p = blockIdx.y;
  const int first = off[p], n = off[p + 1] - first;
  if (n < 2) return;
  const int* v = pts + 2 * (long)first;
  // rows the non-horizontal edges cover, and how many of them there are
  int ymin = INT_MAX, ymax = INT_MIN, n_edges = 0;
  for (int e = lane; e < n; e += 64) {
    const int py = v[2 * (e == 0 ? n - 1 : e - 1) + 1], qy = v[2 * e + 1];
    if (py != qy) {
      ymin = min(ymin, min(py, qy));
      ymax = max(ymax, max(py, qy));
      ++n_edges;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    ymin = min(ymin, __shfl_xor(ymin, o, 64));
    ymax = max(ymax, __shfl_xor(ymax, o, 64));
    n_edges += __shfl_xor(n_edges, o, 64);
  }
  if (n_edges < 2) return;                                    // outline only
  const int rlo = max(ymin, 0), rhi = min(ymax, H);
  unsigned char* plane_out = out + (long)plane[p] * H * W;
  for (int y = rlo + (int)blockIdx.x; y < rhi; y += (int)gridDim.x) {
    int count = 0;
    for (int base = 0; base < n; base += 64) {
      const int e = base + lane;
      bool hit = false;
      long long x = 0;
      if (e < n) {
        const int u = e == 0 ? n - 1 : e - 1;
        const int px = v[2 * u], py = v[2 * u + 1], qx = v[2 * e], qy = v[2 * e + 1];
        const int y0 = min(py, qy), y1 = max(py, qy);
        if (y0 <= y && y < y1) {
          hit = true;
          const long long d = ((long long)(qx - px) * 65536) / (qy - py);      // C division, as cvlite._cdiv
          x = (long long)(py < qy ? px : qx) * 65536 + (long long)(y - y0) * d;
        }
      }
      const unsigned long long m = __ballot(hit);
      if (hit) cross[count + __popcll(m & ((1ULL << lane) - 1ULL))] = x;
      count += __popcll(m);
    }
    __syncthreads();
    // (value, index) order: rank of every crossing and the value that follows it; even ranks open a span
    for (int k = lane; k < count; k += 64) {
      const long long xk = cross[k];
      int rank = 0;
      long long next = LLONG_MAX;
      for (int j = 0; j < count; ++j) {
        const long long xj = cross[j];
        if (xj < xk || (xj == xk && j < k)) ++rank;
        else if (j != k) next = min(next, xj);
      }
      if (!(rank & 1) && rank + 1 < count) {                   // an odd last crossing is dropped
        span[rank] = (int)(xk >> 16);
        span[rank + 1] = (int)(next >> 16);
      }
    }
    __syncthreads();
    unsigned char* row = plane_out + (long)y * W;
    for (int s = 0; s + 1 < count; s += 2) {
      const int x1 = span[s], x2 = span[s + 1];
      if (x1 < W && x2 >= 0) {
        const int hi = min(x2, W - 1);
        for (int x = max(x1, 0) + lane; x <= hi; x += 64) row[x] = 1;
      }
    }
    __syncthreads();                                           // the next row rewrites both lists
  }
}

}  // namespace

// pts / poly_off / poly_plane: HOST arrays (checked here, never read by a kernel); desc_dev: their DEVICE copy, int32
// [poly_off (n_poly + 1) | poly_plane (n_poly) | pts (2 * n_pts)], uploaded by the caller in stream order before this call.
extern "C" int haff_fill_contours_u8(const int* pts, const int* poly_off, const int* poly_plane, const int* desc_dev, int n_poly,
                                     int n_planes, void* out, int H, int W, void* stream) {
  if (n_poly < 0 || n_planes <= 0 || H <= 0 || W <= 0 || H > HAFF_FILL_MAX_COORD || W > HAFF_FILL_MAX_COORD || !out)
    return HAFF_ERR_BAD_ARG;
  int n_pts = 0, max_verts = 0;
  if (n_poly > 0) {
    if (!pts || !poly_off || !poly_plane || !desc_dev || poly_off[0] != 0) return HAFF_ERR_BAD_ARG;
    for (int p = 0; p < n_poly; ++p) {
      const long n = (long)poly_off[p + 1] - poly_off[p];
      if (n < 0 || n > HAFF_FILL_MAX_VERTS || poly_plane[p] < 0 || poly_plane[p] >= n_planes) return HAFF_ERR_BAD_ARG;
      if (n > max_verts) max_verts = (int)n;
    }
    n_pts = poly_off[n_poly];
    if (n_pts > (INT_MAX - 64) / 2) return HAFF_ERR_BAD_ARG;
    for (long i = 0; i < 2L * n_pts; ++i)
      if (pts[i] <= -HAFF_FILL_MAX_COORD || pts[i] >= HAFF_FILL_MAX_COORD) return HAFF_ERR_BAD_ARG;
  }
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (hipMemsetAsync(out, 0, (size_t)n_planes * H * W, s) != hipSuccess) return HAFF_ERR_LAUNCH;
  if (n_pts == 0) return HAFF_OK;
  const int* off_d = desc_dev;
  const int* plane_d = desc_dev + n_poly + 1;
  const int* pts_d = desc_dev + 2 * n_poly + 1;
  const int edge_blocks = (n_pts + 3) / 4;                    // 4 waves per block, one edge per wave
  hipLaunchKernelGGL(outline_kernel, dim3(edge_blocks > 4096 ? 4096 : edge_blocks), dim3(256), 0, s, off_d, plane_d, pts_d, n_poly,
                     n_pts, (unsigned char*)out, H, W);
  if (max_verts >= 2) {
    const int row_groups = H < 128 ? H : 128;
    // polygons ride the grid's y dimension (65535 at most): more than that go out in slices
    for (int p0 = 0; p0 < n_poly; p0 += 65535) {
      const int np = n_poly - p0 < 65535 ? n_poly - p0 : 65535;
      hipLaunchKernelGGL(fill_kernel, dim3(row_groups, np), dim3(64), (size_t)max_verts * 8 + ((size_t)max_verts / 2 + 1) * 8, s,
                         off_d + p0, plane_d + p0, pts_d, (unsigned char*)out, H, W, max_verts);
    }
  }
  return haff_check_launch();
}
