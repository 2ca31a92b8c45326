// Hausdorff distances on the device (ActAffordance/scripts/evaluation/calculate_iou.py:9-24 as evaluation.calculate_hausdorff and
// cvlite.find_contours_external restate it): the contour walk and the point-set distance that used to run in Python per plane.
//
//   haff_contour_hausdorff : for a batch of u8 planes (on = byte != 0, each read as if surrounded by one ring of background) the
//                            CHAIN_APPROX_SIMPLE vertex list of `find_contours_external(plane)[0]`, and for every (bench, pred) pair
//                            of planes the two directed squared Hausdorff distances between those lists. Integers throughout.
//
//   haff_contour_extract   : for the same batch, ALL of `find_contours_external(plane)`: every contour's vertex list, back to back in
//                            OpenCV's order, with an offset table (what a 2HANDS contour record holds). The labelling stages are
//                            shared; its own five follow plan() below.
//
// haff_contour_hausdorff: four stages, six launches on the caller's stream, nothing read back:
//   1 labelling   union-find on int32 parents with a vector atomicMin (Playne-Hawick / Komura). Foreground is 8-connected, background
//                 4-connected: one pass labels both, a pixel only merges with neighbours of its own class. A background pixel on the
//                 plane's edge starts with parent -1 = the ring, so "outside" is the background component whose root is -1. Local
//                 merge of a 32 x 32 tile in LDS (label_tile_kernel), merges across tile edges in HBM (label_seam_kernel), then every
//                 pixel takes its root (label_root_kernel). A parent is always <= its child in raster order and atomicMin only ever
//                 lowers one, so the final roots are the components' raster-first pixels whatever the arrival order.
//   2 start       a candidate is a foreground pixel whose left neighbour is outside; the start pixel of [0] is the maximum over the
//                 candidates of their root (the external component that starts LAST), -1 without one: atomicMax in label_root_kernel.
//   3 walk        cvlite._follow, one wavefront per plane, on a one-bit-per-pixel copy of the plane (written by label_root_kernel,
//                 held in LDS when it fits): lanes 0-7 read the eight neighbours in the search order, a ballot picks the first
//                 that is on, lane 0 appends the vertex. Capped at 8 H W + 8 steps (every (pixel, incoming direction) state
//                 occurs once per cycle): at the cap, or on a step with no neighbour, the plane's fault flag is set and the walk ends.
//   4 distances   d2(A -> B) = max over a of min over b of |a - b|^2, brute force, one workgroup per pair and direction, B staged
//                 through LDS in chunks of kChunk points. Integer min / max only: no order can change a bit of the result.
//
// Every loop is bounded: a find by the plane's pixel count, a merge's retries by twice that (each retry means another thread
// lowered one of the two roots), the walk by its cap. A bound that is hit sets the plane's fault flag: the pair's distances are then
// written as 0 and the caller recomputes the frame on the host.
#include "haff_common.h"

namespace {

constexpr int kMaxSide = 4096;            // coordinates fit int16, d2 <= 2 * 4095^2 fits 32 bits
constexpr int kMaxPlanes = 4096;
constexpr int kMaxPairs = 65535;
constexpr int kMaxVertices = 1 << 22;
constexpr int kTile = 32;                 // label_tile_kernel's tile side (tests/test_hausdorff_kernels_gpu.py names it)
constexpr int kWalkLdsBytes = 128 * 1024; // planes of up to 2^20 pixels are walked in LDS
constexpr int kChunk = 1024;              // points of the inner list per LDS stage (tests name it too)

constexpr unsigned kOverflow = 1u, kFault = 2u;   // per plane; result flags = bench | pred << 2

struct Plane {                            // == haff_contour_plane (include/haff_hip.h)
  const unsigned char* plane;
  int H, W;
};
static_assert(sizeof(Plane) == 16, "descriptor layout");
HAFF_SAME_SIZE(Plane, haff_contour_plane);
HAFF_SAME_FIELD(Plane, plane, haff_contour_plane, plane);
HAFF_SAME_FIELD(Plane, H, haff_contour_plane, H);
HAFF_SAME_FIELD(Plane, W, haff_contour_plane, W);

struct PlaneState {                       // workspace, one per plane
  long label_off;                         // first label of the plane, in ints from the label area's base
  long bits_off;                          // first 64-pixel word of the plane's packed copy (bit k of word j: raster pixel 64 j + k)
  int start;                              // raster index of [0]'s start pixel, -1 = no contour
  int count;                              // vertices of the walk (all of them, also past max_vertices)
  unsigned flags;
  int pad;
};
static_assert(sizeof(PlaneState) == 32, "state layout");

__host__ __device__ inline long align_up(long v, long a) { return (v + a - 1) / a * a; }

// class of a pixel: 1 foreground, 0 background, 2 off the plane (merges with nothing)
__device__ __forceinline__ int pixel_class(const Plane& p, int x, int y) {
  if (x < 0 || y < 0 || x >= p.W || y >= p.H) return 2;
  return p.plane[(long)y * p.W + x] != 0 ? 1 : 0;
}

// root of a: parents only decrease, -1 is the ring. Bounded by n steps; `ok` is cleared when the bound is hit.
__device__ __forceinline__ int uf_find(const int* L, int a, int n, bool& ok) {
  int steps = 0;
  while (a >= 0) {
    const int b = __hip_atomic_load(L + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (b == a) break;
    a = b;
    if (++steps > n) { ok = false; break; }
  }
  return a;
}

__device__ __forceinline__ void uf_merge(int* L, int a, int b, int n, bool& ok) {
  for (int tries = 0; tries <= 2 * n + 2; ++tries) {
    a = uf_find(L, a, n, ok);
    b = uf_find(L, b, n, ok);
    if (a == b || !ok) return;
    if (a < b) { const int t = a; a = b; b = t; }        // a > b >= -1: hang the larger root under the smaller
    const int old = atomicMin(L + a, b);
    if (old == a) return;
    a = old;
  }
  ok = false;
}

__global__ void ch_setup_kernel(const Plane* planes, int n_planes, PlaneState* st) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n_planes) return;
  long off = 0, words = 0;
  for (int q = 0; q < p; ++q) {
    const long n = (long)planes[q].H * planes[q].W;
    off += align_up(n, 4);
    words += (n + 63) / 64;
  }
  PlaneState s;
  s.label_off = off;
  s.bits_off = words;
  s.start = -1;
  s.count = 0;
  s.flags = 0u;
  s.pad = 0;
  st[p] = s;
}

// stage 1a: one 32 x 32 tile per workgroup, 256 threads x 4 pixels; parents are tile-local raster indices in LDS.
// Which neighbour pairs are merged (here and in label_seam_kernel; x-1 = L, y-1 = U, and UL, UR): L always; U unless L and UL are
// of the pixel's class too (then L, or a pixel further left in the run, has joined the two rows); for a foreground pixel whose U
// is not foreground, UL unless L is foreground (L's U), and UR. A neighbour outside the tile counts as unknown here, which only
// ever adds a merge. The L merges cost no atomics: every pixel starts at the first pixel of its row run, found with a ballot.
__global__ __launch_bounds__(256) void label_tile_kernel(const Plane* planes, PlaneState* st, int* labels) {
  __shared__ int L[kTile * kTile];
  __shared__ unsigned char cls[kTile * kTile];
  const Plane pl = planes[blockIdx.y];
  const int tiles_x = (pl.W + kTile - 1) / kTile, tiles_y = (pl.H + kTile - 1) / kTile;
  if ((int)blockIdx.x >= tiles_x * tiles_y) return;       // a smaller plane of the batch: the whole workgroup leaves
  const int x0 = ((int)blockIdx.x % tiles_x) * kTile, y0 = ((int)blockIdx.x / tiles_x) * kTile;
  const int lx = threadIdx.x & (kTile - 1), ly0 = threadIdx.x / kTile, lane = threadIdx.x & 63;
  int* out = labels + st[blockIdx.y].label_off;
  bool ok = true;
  for (int k = 0; k < 4; ++k) {
    const int ly = ly0 + 8 * k;
    cls[ly * kTile + lx] = (unsigned char)pixel_class(pl, x0 + lx, y0 + ly);
  }
  __syncthreads();
  int run[4];
  for (int k = 0; k < 4; ++k) {                            // a wave holds two rows of the tile: lanes 0-31 and 32-63
    const int ly = ly0 + 8 * k, i = ly * kTile + lx, x = x0 + lx, y = y0 + ly;
    const int c = cls[i];
    const unsigned long long heads = __ballot(lx == 0 || cls[i - 1] != c);
    const int head = 63 - __clzll((long long)(heads & ((2ull << lane) - 1ull)));   // lanes 0 and 32 are heads: never empty
    run[k] = i - (lane - head);
    const bool edge = x == 0 || y == 0 || x == pl.W - 1 || y == pl.H - 1;
    L[i] = (c == 0 && edge) ? -1 : run[k];
  }
  __syncthreads();
  for (int k = 0; k < 4; ++k) {
    const int ly = ly0 + 8 * k, i = ly * kTile + lx, x = x0 + lx, y = y0 + ly;
    const int c = cls[i];
    if (c == 2) continue;
    if (c == 0 && run[k] != i && (x == pl.W - 1 || y == pl.H - 1)) uf_merge(L, run[k], -1, kTile * kTile, ok);   // the run reaches the ring
    if (ly == 0) continue;
    const int cu = cls[i - kTile], cl = lx > 0 ? cls[i - 1] : 2, cul = lx > 0 ? cls[i - kTile - 1] : 2;
    const int cur = lx < kTile - 1 ? cls[i - kTile + 1] : 2;
    if (cu == c && !(cl == c && cul == c)) uf_merge(L, i, i - kTile, kTile * kTile, ok);
    if (c == 1 && cu != 1) {
      if (cul == 1 && cl != 1) uf_merge(L, i, i - kTile - 1, kTile * kTile, ok);
      if (cur == 1) uf_merge(L, i, i - kTile + 1, kTile * kTile, ok);
    }
  }
  __syncthreads();
  for (int k = 0; k < 4; ++k) {
    const int ly = ly0 + 8 * k, i = ly * kTile + lx;
    if (cls[i] == 2) continue;
    const int r = uf_find(L, i, kTile * kTile, ok);
    out[(long)(y0 + ly) * pl.W + x0 + lx] = r < 0 ? -1 : (y0 + r / kTile) * pl.W + x0 + (r & (kTile - 1));
  }
  if (!ok) atomicOr(&st[blockIdx.y].flags, kFault);
}

// stage 1b: the pairs of label_tile_kernel's rule that straddle a tile edge, decided on the plane itself
__global__ __launch_bounds__(256) void label_seam_kernel(const Plane* planes, PlaneState* st, int* labels) {
  const Plane pl = planes[blockIdx.y];
  const int tiles_x = (pl.W + kTile - 1) / kTile, tiles_y = (pl.H + kTile - 1) / kTile;
  if ((int)blockIdx.x >= tiles_x * tiles_y) return;
  const int x0 = ((int)blockIdx.x % tiles_x) * kTile, y0 = ((int)blockIdx.x / tiles_x) * kTile;
  const int lx = threadIdx.x & (kTile - 1), ly0 = threadIdx.x / kTile;
  int* L = labels + st[blockIdx.y].label_off;
  const int n = pl.H * pl.W;
  bool ok = true;
  for (int k = 0; k < 4; ++k) {
    const int ly = ly0 + 8 * k, x = x0 + lx, y = y0 + ly;
    if (lx != 0 && ly != 0 && lx != kTile - 1) continue;  // every neighbour above is in this tile
    const int c = pixel_class(pl, x, y);
    if (c == 2) continue;
    const int i = y * pl.W + x;
    const int cl = pixel_class(pl, x - 1, y), cu = pixel_class(pl, x, y - 1), cul = pixel_class(pl, x - 1, y - 1);
    if (lx == 0 && cl == c) uf_merge(L, i, i - 1, n, ok);
    if (ly == 0 && cu == c && !(cl == c && cul == c)) uf_merge(L, i, i - pl.W, n, ok);
    if (c == 1 && cu != 1) {
      if ((lx == 0 || ly == 0) && cul == 1 && cl != 1) uf_merge(L, i, i - pl.W - 1, n, ok);
      if ((lx == kTile - 1 || ly == 0) && pixel_class(pl, x + 1, y - 1) == 1) uf_merge(L, i, i - pl.W + 1, n, ok);
    }
  }
  if (!ok) atomicOr(&st[blockIdx.y].flags, kFault);
}

// stages 1c and 2: every pixel takes its root; a foreground pixel whose left neighbour is outside offers its root as the start.
// Also packs the plane, one bit per pixel in raster order, for the walk.
__global__ __launch_bounds__(256) void label_root_kernel(const Plane* planes, PlaneState* st, int* labels,
                                                         unsigned long long* bits) {
  const Plane pl = planes[blockIdx.y];
  const int n = pl.H * pl.W;
  int* L = labels + st[blockIdx.y].label_off;
  unsigned long long* packed = bits + st[blockIdx.y].bits_off;
  bool ok = true;
  int best = -1;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    const int r = uf_find(L, i, n, ok);
    // a store of an ancestor: a find that runs beside it still ends at the same root
    __hip_atomic_store(L + i, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool on = pl.plane[i] != 0;
    const unsigned long long word = __ballot(on);         // a wave's 64 pixels are consecutive and start at a multiple of 64
    if ((threadIdx.x & 63) == 0) packed[i >> 6] = word;
    if (!on) continue;
    const int x = i % pl.W;
    const bool cand = x == 0 || (pl.plane[i - 1] == 0 && uf_find(L, i - 1, n, ok) == -1);
    if (cand && r > best) best = r;
  }
  if (best >= 0 && best > __hip_atomic_load(&st[blockIdx.y].start, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
    atomicMax(&st[blockIdx.y].start, best);
  if (!ok) atomicOr(&st[blockIdx.y].flags, kFault);
}

// codes 0 = +x, 1 = +x-y, 2 = -y, ... 7 = +x+y (y down), as cvlite._DX / _DY
__device__ __forceinline__ int dir_dx(int s) { return (s == 0 || s == 1 || s == 7) ? 1 : (s == 3 || s == 4 || s == 5) ? -1 : 0; }
__device__ __forceinline__ int dir_dy(int s) { return (s == 1 || s == 2 || s == 3) ? -1 : (s == 5 || s == 6 || s == 7) ? 1 : 0; }

__device__ __forceinline__ bool bit_on(const unsigned long long* bits, int H, int W, int x, int y) {
  if (x < 0 || y < 0 || x >= W || y >= H) return false;
  const int b = y * W + x;
  return (bits[b >> 6] >> (b & 63)) & 1ull;
}

// cvlite._follow from (x0, y0) on the packed plane, one wavefront: every lane carries the walk's state (it is wave-uniform), lanes
// 0-7 probe. Returns the vertex count; `flags` collects overflow and fault. kStore = false only counts: nothing is written and
// nothing overflows (haff_contour_extract's first walk).
template <bool kStore = true>
__device__ __forceinline__ int follow(const unsigned long long* bits, int H, int W, int x0, int y0, short2* out, int max_vertices,
                                      int lane, unsigned& flags) {
  // the first foreground neighbour clockwise from "left": s = 3, 2, 1, 0, 7, 6, 5 (4, the left one, is background)
  const int s_probe = (3 - lane) & 7;
  const unsigned long long m0 = __ballot(lane < 7 && bit_on(bits, H, W, x0 + dir_dx(s_probe), y0 + dir_dy(s_probe)));
  if (m0 == 0ull) {                                       // an isolated pixel
    if (kStore && lane == 0) out[0] = make_short2((short)x0, (short)y0);
    return 1;
  }
  int nv = 0;
  int s = (3 - (__ffsll((long long)m0) - 1)) & 7;
  const int x1 = x0 + dir_dx(s), y1 = y0 + dir_dy(s);
  int x3 = x0, y3 = y0, prev_s = s ^ 4;
  const int cap = 8 * H * W + 8;
  for (int step = 0;; ++step) {
    if (step >= cap) { flags |= kFault; break; }
    const int sk = (s + 1 + lane) & 7;                    // counter-clockwise from the direction we came from
    const unsigned long long m = __ballot(lane < 8 && bit_on(bits, H, W, x3 + dir_dx(sk), y3 + dir_dy(sk)));
    if (m == 0ull) { flags |= kFault; break; }            // cannot happen after a found neighbour: never spin on it
    s = (s + 1 + (__ffsll((long long)m) - 1)) & 7;
    const int x4 = x3 + dir_dx(s), y4 = y3 + dir_dy(s);
    if (s != prev_s) {
      if (kStore) {
        if (nv < max_vertices) {
          if (lane == 0) out[nv] = make_short2((short)x3, (short)y3);
        } else {
          flags |= kOverflow;
        }
      }
      ++nv;
      prev_s = s;
    }
    if (x4 == x0 && y4 == y0 && x3 == x1 && y3 == y1) break;
    x3 = x4;
    y3 = y4;
    s = (s + 4) & 7;
  }
  return nv;
}

// stage 3: one workgroup per plane. Its four waves copy the packed plane into LDS when it fits (lds_words; an 855 x 855 plane is
// 91 KB), then wave 0 walks: one LDS read per step instead of a trip to L2. A larger plane is walked on the packed copy in HBM.
__global__ __launch_bounds__(256) void contour_walk_kernel(const Plane* planes, PlaneState* st, const unsigned long long* bits,
                                                           short2* verts, int* counts, int max_vertices, int lds_words) {
  extern __shared__ unsigned long long lds_bits[];
  const int p = blockIdx.x, tid = threadIdx.x;
  const Plane pl = planes[p];
  const int start = st[p].start;                          // uniform over the workgroup
  if (start < 0) {
    if (tid == 0) counts[p] = 0;
    return;
  }
  const unsigned long long* packed = bits + st[p].bits_off;
  const int words = (pl.H * pl.W + 63) / 64;
  const bool in_lds = words <= lds_words;
  if (in_lds) {
    for (int j = tid; j < words; j += 256) lds_bits[j] = packed[j];
    __syncthreads();
  }
  if (tid >= 64) return;
  short2* out = verts + (long)p * max_vertices;
  unsigned flags = 0u;
  const int x0 = start % pl.W, y0 = start / pl.W;
  const int nv = in_lds ? follow(lds_bits, pl.H, pl.W, x0, y0, out, max_vertices, tid, flags)
                        : follow(packed, pl.H, pl.W, x0, y0, out, max_vertices, tid, flags);
  if (tid == 0) {
    st[p].count = nv;
    if (flags) atomicOr(&st[p].flags, flags);
    counts[p] = nv;
  }
}

// stage 4: grid (pairs, 2). y = 0: d2(pred -> bench) and the pair's record; y = 1: d2(bench -> pred)
__global__ __launch_bounds__(256) void hausdorff_d2_kernel(const int* pairs, const PlaneState* st, const short2* verts,
                                                           int max_vertices, unsigned* result) {
  __shared__ short2 stage[kChunk];
  __shared__ int red[4];
  const int pair = blockIdx.x, dir = blockIdx.y, tid = threadIdx.x;
  const int bench = pairs[2 * pair], pred = pairs[2 * pair + 1];
  const PlaneState sb = st[bench], sp = st[pred];
  const unsigned flags = sb.flags | (sp.flags << 2);
  unsigned* res = result + (long)pair * 6;
  if (dir == 0 && tid == 0) {
    res[0] = (unsigned)sb.count;
    res[1] = (unsigned)sp.count;
    res[4] = flags;
    res[5] = 0u;
  }
  if (flags != 0u || sb.count == 0 || sp.count == 0) {    // uniform over the workgroup
    if (tid == 0) res[2 + dir] = 0u;
    return;
  }
  const int outer_plane = dir == 0 ? pred : bench, inner_plane = dir == 0 ? bench : pred;
  const int n_outer = dir == 0 ? sp.count : sb.count, n_inner = dir == 0 ? sb.count : sp.count;
  const short2* A = verts + (long)outer_plane * max_vertices;
  const short2* B = verts + (long)inner_plane * max_vertices;
  int mx = 0;
  for (int base = 0; base < n_outer; base += 256) {       // uniform trip counts: every thread meets every barrier
    const bool live = base + tid < n_outer;
    const short2 a = live ? A[base + tid] : make_short2(0, 0);
    int mn = 0x7fffffff;
    for (int c0 = 0; c0 < n_inner; c0 += kChunk) {
      const int len = n_inner - c0 < kChunk ? n_inner - c0 : kChunk;
      __syncthreads();
      for (int j = tid; j < len; j += 256) stage[j] = B[c0 + j];
      __syncthreads();
      for (int j = 0; j < len; ++j) {
        const short2 b = stage[j];
        const int dx = (int)a.x - (int)b.x, dy = (int)a.y - (int)b.y;
        const int d = dx * dx + dy * dy;
        mn = d < mn ? d : mn;
      }
    }
    if (live && mn > mx) mx = mn;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int v = __shfl_xor(mx, o, 64);
    mx = v > mx ? v : mx;
  }
  if ((tid & 63) == 0) red[tid >> 6] = mx;
  __syncthreads();
  if (tid == 0) {
    int m = red[0];
    for (int w = 1; w < 4; ++w) m = red[w] > m ? red[w] : m;
    res[2 + dir] = (unsigned)m;
  }
}

// the workspace's areas (byte offsets) and what the launches need of the plane table
struct Layout {
  long labels, bits, state, verts, counts, total;
  long words;                             // 64-pixel words of all packed planes
  int max_tiles, rb;                      // the labelling grids' x: tiles of the largest plane, label_root_kernel's workgroups
  int lds_words;                          // the walk's LDS: the largest packed plane of the batch that fits kWalkLdsBytes
};

// 0, or the refusal code of the plane table / max_vertices
int plan(const Plane* pl, int n_planes, int max_vertices, Layout& lay) {
  if (!pl || n_planes <= 0 || n_planes > kMaxPlanes) return HAFF_ERR_BAD_ARG;
  if (!haff_aligned(pl, 8)) return HAFF_ERR_BAD_ARG;
  if (max_vertices < 1 || max_vertices > kMaxVertices) return HAFF_ERR_BAD_ARG;
  long ints = 0, max_pixels = 1;
  lay.words = 0;
  lay.max_tiles = 1;
  lay.lds_words = 0;
  for (int i = 0; i < n_planes; ++i) {
    if (pl[i].H <= 0 || pl[i].W <= 0) return HAFF_ERR_BAD_ARG;
    if (pl[i].H > kMaxSide || pl[i].W > kMaxSide) return HAFF_ERR_UNSUPPORTED;
    const long n = (long)pl[i].H * pl[i].W, w = (n + 63) / 64;
    ints += align_up(n, 4);
    lay.words += w;
    if (w * 8 <= kWalkLdsBytes && w > lay.lds_words) lay.lds_words = (int)w;
    const int t = ((pl[i].W + kTile - 1) / kTile) * ((pl[i].H + kTile - 1) / kTile);
    lay.max_tiles = t > lay.max_tiles ? t : lay.max_tiles;
    max_pixels = n > max_pixels ? n : max_pixels;
  }
  const long rb = (max_pixels + 256L * 4 - 1) / (256L * 4);
  lay.rb = rb > 256 ? 256 : (int)rb;
  lay.labels = 0;
  lay.bits = align_up(ints * 4, 16);
  lay.state = align_up(lay.bits + lay.words * 8, 16);
  lay.verts = align_up(lay.state + (long)n_planes * (long)sizeof(PlaneState), 16);
  lay.counts = lay.verts + (long)n_planes * max_vertices * 4;
  lay.total = align_up(lay.counts + (long)n_planes * 4, 16);
  return HAFF_OK;
}

struct Labelled { int* labels; unsigned long long* bits; PlaneState* st; };

// stages 1a-1c (and 2) on the caller's stream: the three areas both entry points share, labelled and packed
Labelled launch_labelling(const Layout& lay, char* ws, const Plane* pd, int n_planes, hipStream_t s) {
  const Labelled l{reinterpret_cast<int*>(ws + lay.labels), reinterpret_cast<unsigned long long*>(ws + lay.bits),
                   reinterpret_cast<PlaneState*>(ws + lay.state)};
  const dim3 tiles((unsigned)lay.max_tiles, (unsigned)n_planes);
  hipLaunchKernelGGL(ch_setup_kernel, dim3((unsigned)((n_planes + 255) / 256)), dim3(256), 0, s, pd, n_planes, l.st);
  hipLaunchKernelGGL(label_tile_kernel, tiles, dim3(256), 0, s, pd, l.st, l.labels);
  hipLaunchKernelGGL(label_seam_kernel, tiles, dim3(256), 0, s, pd, l.st, l.labels);
  hipLaunchKernelGGL(label_root_kernel, dim3((unsigned)lay.rb, (unsigned)n_planes), dim3(256), 0, s, pd, l.st, l.labels, l.bits);
  return l;
}

// a walk kernel may take kWalkLdsBytes of dynamic LDS
template <typename K> bool allow_walk_lds(K kernel) {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, kWalkLdsBytes) ==
         hipSuccess;
}

// ---- haff_contour_extract: every external contour of every plane (cvlite.find_contours_external, all of it) -------------------
// Stages 1a-1c above label the planes. Then, each stage a launch of its own, ordered by the stream alone:
//   starts   a contour starts at every foreground pixel that is its component's root and has x == 0 or an outside left neighbour
//            (the root of an external component is always such a pixel: tests/contours_ref.py restates the rule): one bit per pixel, by ballot.
//   number   one workgroup per plane counts the start bits in DESCENDING raster order (OpenCV's order): contour k's start pixel.
//   count    one wavefront per contour walks it with follow<false>: the contour's vertex count.
//   offsets  one workgroup per plane: exclusive scan of the counts, the summary row, the flags.
//   write    the count walk again, storing at the contour's offset; skipped for a flagged plane.
constexpr int kMaxContours = 1 << 22;
constexpr unsigned kTooMany = 4u;         // summary flags: kOverflow, kFault, and more contours than max_contours
constexpr int kWalkGrid = 64;             // workgroups per plane of the two walks: 4 contours each, then strided

__global__ __launch_bounds__(256) void extract_start_kernel(const Plane* planes, const PlaneState* st, const int* labels,
                                                            unsigned long long* start_bits) {
  const Plane pl = planes[blockIdx.y];
  const int n = pl.H * pl.W;
  const int* L = labels + st[blockIdx.y].label_off;       // final roots: label_root_kernel has run
  unsigned long long* marks = start_bits + st[blockIdx.y].bits_off;
  for (int i = blockIdx.x * 256 + threadIdx.x; i < n; i += gridDim.x * 256) {
    bool mark = pl.plane[i] != 0 && L[i] == i;
    if (mark && i % pl.W != 0) mark = pl.plane[i - 1] == 0 && L[i - 1] == -1;
    const unsigned long long word = __ballot(mark);       // as in label_root_kernel: a wave's 64 pixels are one word
    if ((threadIdx.x & 63) == 0) marks[i >> 6] = word;
  }
}

// exclusive scan of one value per thread over the workgroup's 256 threads; *total = the sum. All threads call it.
__device__ __forceinline__ unsigned block_exclusive_scan(unsigned v, unsigned* total) {
  __shared__ unsigned wave_sum[4];
  __shared__ unsigned sum_all;
  const int tid = threadIdx.x, lane = tid & 63;
  unsigned inc = v;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned u = __shfl_up(inc, o, 64);
    if (lane >= o) inc += u;
  }
  __syncthreads();                                        // a second call: the last one's reads are over
  if (lane == 63) wave_sum[tid >> 6] = inc;
  __syncthreads();
  unsigned base = 0u;
  for (int w = 0; w < (tid >> 6); ++w) base += wave_sum[w];
  if (tid == 255) sum_all = base + inc;
  __syncthreads();
  *total = sum_all;
  return base + inc - v;
}

// thread t takes the words [words - 1 - t * per, ...) downwards, `per` of them: descending raster order over the workgroup
__global__ __launch_bounds__(256) void extract_number_kernel(const Plane* planes, const PlaneState* st,
                                                             const unsigned long long* start_bits, int* starts, int* n_contours,
                                                             int max_contours) {
  const int p = blockIdx.x, tid = threadIdx.x;
  const int words = (planes[p].H * planes[p].W + 63) / 64;
  const unsigned long long* marks = start_bits + st[p].bits_off;
  const int per = (words + 255) / 256;
  const int first = words - 1 - tid * per;                // may be < 0: the thread has no words
  int last = first - per + 1;
  last = last < 0 ? 0 : last;
  unsigned mine = 0u;
  for (int j = first; j >= last; --j) mine += (unsigned)__popcll(marks[j]);
  unsigned total;                                         // at most H W <= 2^24
  int k = (int)block_exclusive_scan(mine, &total);
  if (tid == 0) n_contours[p] = (int)total;
  int* out = starts + (long)p * max_contours;
  for (int j = first; j >= last && k < max_contours; --j) {
    unsigned long long w = marks[j];
    while (w != 0ull && k < max_contours) {               // at most 64 rounds: a bit leaves every round
      const int b = 63 - __clzll((long long)w);
      out[k++] = 64 * j + b;
      w &= ~(1ull << b);
    }
  }
}

template <bool kStore>
__global__ __launch_bounds__(256) void extract_walk_kernel(const Plane* planes, PlaneState* st, const unsigned long long* bits,
                                                           const int* starts, const int* n_contours, int* counts, const int* offsets,
                                                           int* summary, short2* verts, int max_contours, int max_vertices,
                                                           int lds_words) {
  extern __shared__ unsigned long long lds_bits[];
  const int p = blockIdx.y, tid = threadIdx.x, lane = tid & 63;
  int nc = n_contours[p];                                 // uniform over the workgroup, as is everything up to the barrier
  if (nc > max_contours) return;                          // kTooMany: nothing of the plane is walked
  if ((int)blockIdx.x * 4 >= nc) return;
  if (kStore) {                                           // a flagged plane is the host's. One read for the workgroup: another
    __shared__ int flagged;                               // workgroup's walk may set the fault bit between two threads' reads
    if (tid == 0) flagged = summary[4 * p + 2];
    __syncthreads();
    if (flagged != 0) return;
  }
  const Plane pl = planes[p];
  const unsigned long long* packed = bits + st[p].bits_off;
  const int words = (pl.H * pl.W + 63) / 64;
  const bool in_lds = words <= lds_words;
  if (in_lds) {
    for (int j = tid; j < words; j += 256) lds_bits[j] = packed[j];
    __syncthreads();
  }
  const int* start = starts + (long)p * max_contours;
  int* count = counts + (long)p * max_contours;
  const int* offs = offsets + (long)p * (max_contours + 1);
  for (int k = (int)blockIdx.x * 4 + (tid >> 6); k < nc; k += (int)gridDim.x * 4) {   // at most max_contours rounds
    const int s = start[k], x0 = s % pl.W, y0 = s / pl.W;
    unsigned flags = 0u;
    if (kStore) {
      const int room = count[k];                          // the count walk's: the walk is the same, so nothing overflows
      short2* out = verts + (long)p * max_vertices + offs[k];
      const int nv = in_lds ? follow<true>(lds_bits, pl.H, pl.W, x0, y0, out, room, lane, flags)
                            : follow<true>(packed, pl.H, pl.W, x0, y0, out, room, lane, flags);
      if (nv != room) flags |= kFault;
      if (flags && lane == 0) atomicOr(reinterpret_cast<unsigned*>(summary) + 4 * p + 2, kFault);
    } else {
      const int nv = in_lds ? follow<false>(lds_bits, pl.H, pl.W, x0, y0, nullptr, 0, lane, flags)
                            : follow<false>(packed, pl.H, pl.W, x0, y0, nullptr, 0, lane, flags);
      if (lane == 0) {
        count[k] = nv;
        if (flags) atomicOr(&st[p].flags, flags);
      }
    }
  }
}

__global__ __launch_bounds__(256) void extract_offsets_kernel(const PlaneState* st, const int* n_contours, const int* counts,
                                                              int* offsets, int* summary, int max_contours, int max_vertices) {
  const int p = blockIdx.x, tid = threadIdx.x;
  const int nc = n_contours[p];
  unsigned flags = st[p].flags & kFault;
  if (nc > max_contours) {                                // uniform: the counts were never made
    if (tid == 0) {
      summary[4 * p] = nc;
      summary[4 * p + 1] = 0;
      summary[4 * p + 2] = (int)(flags | kTooMany);
      summary[4 * p + 3] = 0;
    }
    return;
  }
  const int* count = counts + (long)p * max_contours;
  int* offs = offsets + (long)p * (max_contours + 1);
  const int per = (nc + 255) / 256;
  const int lo = tid * per < nc ? tid * per : nc, hi = lo + per < nc ? lo + per : nc;
  // the contours are disjoint sets of (pixel, direction) states: without a fault the plane's total is at most 8 H W <= 2^27.
  // A faulted walk's counts may sum past 2^31: unsigned sums, and the plane is flagged whatever they come to.
  unsigned mine = 0u;
  for (int k = lo; k < hi; ++k) mine += (unsigned)count[k];
  unsigned total;
  unsigned run = block_exclusive_scan(mine, &total);
  for (int k = lo; k < hi; ++k) {
    offs[k] = (int)run;
    run += (unsigned)count[k];
  }
  if (tid == 0) {
    if (total > (unsigned)max_vertices) flags |= kOverflow;
    offs[nc] = (int)total;
    summary[4 * p] = nc;
    summary[4 * p + 1] = (int)total;
    summary[4 * p + 2] = (int)flags;
    summary[4 * p + 3] = 0;
  }
}

struct ExtractLayout { long start_bits, starts, counts, n_contours, total; };

// plan()'s refusals, max_contours, and the extract stages' areas behind the labelling's (lay.verts is where plan()'s own end)
int plan_extract(const Plane* pl, int n_planes, int max_contours, int max_vertices, Layout& lay, ExtractLayout& ext) {
  const int rc = plan(pl, n_planes, max_vertices, lay);
  if (rc != HAFF_OK) return rc;
  if (max_contours < 1 || max_contours > kMaxContours) return HAFF_ERR_BAD_ARG;
  ext.start_bits = lay.verts;
  ext.starts = align_up(ext.start_bits + lay.words * 8, 16);
  ext.counts = align_up(ext.starts + (long)n_planes * max_contours * 4, 16);
  ext.n_contours = align_up(ext.counts + (long)n_planes * max_contours * 4, 16);
  ext.total = align_up(ext.n_contours + (long)n_planes * 4, 16);
  return HAFF_OK;
}

}  // namespace

extern "C" int haff_contour_extract_workspace(const void* planes_host, int n_planes, int max_contours, int max_vertices,
                                              long* bytes_out) {
  if (!bytes_out) return HAFF_ERR_BAD_ARG;
  Layout lay;
  ExtractLayout ext;
  const int rc = plan_extract(static_cast<const Plane*>(planes_host), n_planes, max_contours, max_vertices, lay, ext);
  if (rc != HAFF_OK) return rc;
  *bytes_out = ext.total;
  return HAFF_OK;
}

extern "C" int haff_contour_extract(const void* planes_host, const void* planes_dev, int n_planes, int max_contours, int max_vertices,
                                    void* workspace, long workspace_bytes, void* verts, void* offsets, void* summary, void* stream) {
  if (!planes_host || !planes_dev || !workspace || !verts || !offsets || !summary) return HAFF_ERR_BAD_ARG;
  Layout lay;
  ExtractLayout ext;
  const int rc = plan_extract(static_cast<const Plane*>(planes_host), n_planes, max_contours, max_vertices, lay, ext);
  if (rc != HAFF_OK) return rc;
  if (!haff_aligned(planes_dev, 8) || !haff_aligned(workspace, 16) || !haff_aligned(verts, 4) || !haff_aligned(offsets, 4) ||
      !haff_aligned(summary, 4))
    return HAFF_ERR_BAD_ARG;
  if (workspace_bytes < ext.total) return HAFF_ERR_BAD_ARG;
  char* ws = static_cast<char*>(workspace);
  unsigned long long* start_bits = reinterpret_cast<unsigned long long*>(ws + ext.start_bits);
  int* starts = reinterpret_cast<int*>(ws + ext.starts);
  int* counts = reinterpret_cast<int*>(ws + ext.counts);
  int* n_contours = reinterpret_cast<int*>(ws + ext.n_contours);
  const Plane* pd = static_cast<const Plane*>(planes_dev);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (!allow_walk_lds(extract_walk_kernel<false>) || !allow_walk_lds(extract_walk_kernel<true>)) return HAFF_ERR_LAUNCH;
  const dim3 roots((unsigned)lay.rb, (unsigned)n_planes);
  int wg = (max_contours + 3) / 4;
  wg = wg > kWalkGrid ? kWalkGrid : wg;
  const dim3 walks((unsigned)wg, (unsigned)n_planes);
  const size_t lds = (size_t)lay.lds_words * 8;
  int* offs = static_cast<int*>(offsets);
  int* sum = static_cast<int*>(summary);
  short2* v = static_cast<short2*>(verts);
  const Labelled l = launch_labelling(lay, ws, pd, n_planes, s);
  hipLaunchKernelGGL(extract_start_kernel, roots, dim3(256), 0, s, pd, l.st, l.labels, start_bits);
  hipLaunchKernelGGL(extract_number_kernel, dim3((unsigned)n_planes), dim3(256), 0, s, pd, l.st, start_bits, starts, n_contours,
                     max_contours);
  hipLaunchKernelGGL(extract_walk_kernel<false>, walks, dim3(256), lds, s, pd, l.st, l.bits, starts, n_contours, counts, offs, sum, v,
                     max_contours, max_vertices, lay.lds_words);
  hipLaunchKernelGGL(extract_offsets_kernel, dim3((unsigned)n_planes), dim3(256), 0, s, l.st, n_contours, counts, offs, sum,
                     max_contours, max_vertices);
  hipLaunchKernelGGL(extract_walk_kernel<true>, walks, dim3(256), lds, s, pd, l.st, l.bits, starts, n_contours, counts, offs, sum, v,
                     max_contours, max_vertices, lay.lds_words);
  return haff_check_launch();
}

extern "C" int haff_contour_hausdorff_workspace(const void* planes_host, int n_planes, int max_vertices, long* bytes_out) {
  if (!bytes_out) return HAFF_ERR_BAD_ARG;
  Layout lay;
  const int rc = plan(static_cast<const Plane*>(planes_host), n_planes, max_vertices, lay);
  if (rc != HAFF_OK) return rc;
  *bytes_out = lay.total;
  return HAFF_OK;
}

extern "C" int haff_contour_hausdorff(const void* planes_host, const void* planes_dev, int n_planes, const int* pairs_host,
                                      const int* pairs_dev, int n_pairs, int max_vertices, void* workspace, long workspace_bytes,
                                      void* verts_out, void* result, void* stream) {
  if (!planes_host || !planes_dev || !pairs_host || !pairs_dev || !result || !workspace) return HAFF_ERR_BAD_ARG;
  if (n_pairs <= 0 || n_pairs > kMaxPairs) return HAFF_ERR_BAD_ARG;
  Layout lay;
  const Plane* pl = static_cast<const Plane*>(planes_host);
  const int rc = plan(pl, n_planes, max_vertices, lay);
  if (rc != HAFF_OK) return rc;
  if (!haff_aligned(planes_dev, 8) || !haff_aligned(pairs_host, 4) || !haff_aligned(pairs_dev, 4) || !haff_aligned(result, 4) ||
      !haff_aligned(workspace, 16) || !haff_aligned(verts_out, 4))
    return HAFF_ERR_BAD_ARG;
  if (workspace_bytes < lay.total) return HAFF_ERR_BAD_ARG;
  for (int i = 0; i < n_pairs; ++i) {
    const int b = pairs_host[2 * i], p = pairs_host[2 * i + 1];
    if (b < 0 || b >= n_planes || p < 0 || p >= n_planes) return HAFF_ERR_BAD_ARG;
    if (pl[b].H != pl[p].H || pl[b].W != pl[p].W) return HAFF_ERR_BAD_ARG;
  }
  char* ws = static_cast<char*>(workspace);
  short2* verts = reinterpret_cast<short2*>(verts_out ? static_cast<char*>(verts_out) : ws + lay.verts);
  int* counts = reinterpret_cast<int*>(verts_out ? static_cast<char*>(verts_out) + (long)n_planes * max_vertices * 4 : ws + lay.counts);
  const Plane* pd = static_cast<const Plane*>(planes_dev);
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  if (!allow_walk_lds(contour_walk_kernel)) return HAFF_ERR_LAUNCH;
  const Labelled l = launch_labelling(lay, ws, pd, n_planes, s);
  hipLaunchKernelGGL(contour_walk_kernel, dim3((unsigned)n_planes), dim3(256), (size_t)lay.lds_words * 8, s, pd, l.st, l.bits, verts,
                     counts, max_vertices, lay.lds_words);
  hipLaunchKernelGGL(hausdorff_d2_kernel, dim3((unsigned)n_pairs, 2u), dim3(256), 0, s, pairs_dev, l.st, verts, max_vertices,
                     static_cast<unsigned*>(result));
  return haff_check_launch();
}
