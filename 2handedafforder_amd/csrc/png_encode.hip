// uint8 greyscale planes -> the DEFLATE block of their PNG stream, on the device (include/haff_io.h states the format; png.py wraps
// the container around it on the host). The planes the command lines write are 0/255 masks, so they are runs: a fixed-Huffman
// block of "literal, then repeat the previous byte n times" tokens is a few KB where the plane is hundreds, and the host reads that
// back instead of the plane and never runs an encoder.
//
// Two calls. haff_png_measure: one wave per scanline finds the run starts (a byte that differs from its left neighbour), prices
// each run with the closed form of the token rule and sums the scanline's Adler terms; one wave per plane then turns the scanline
// bit counts into bit offsets (exclusive scan from the 3 header bits) and writes the plane's length and Adler-32; one wave lays the
// planes back to back. haff_png_emit: the same walk, with a wave scan of the run costs inside the scanline, and every lane that
// closes a run ORs its tokens into place. Neighbouring runs and scanlines share words, hence atomicOr on 32-bit words; OR is
// order-independent, so the bytes are a function of the plane alone.
#include "haff_common.h"
#include "haff_io.h"

namespace {

constexpr int kMaxSide = 4096;            // a scanline's B_y (<= 255 S (S + 1) / 2) and a plane's bit count (<= 10 + 9 S H) fit 32 bits
constexpr int kMaxPlanes = 4096;
constexpr long kMaxBytes = 1L << 31;      // of the worst-case blocks of one call: the table's byte offsets are 32-bit
constexpr unsigned kAdler = 65521u;
constexpr int kRowWaves = 4;              // scanlines per 256-thread workgroup
constexpr unsigned kMatch258 = 0xA3u;     // length symbol 285 (code 11000101, first bit in bit 0), then five zero distance bits: 13 bits
constexpr unsigned kMatch258Bits = 13;

typedef haff_png_plane Plane;

// m = 3 .. 258 -> the match (length m, distance 1) as it enters the stream: bits 0..23 = the length symbol's Huffman code with its
// first bit in bit 0, the extra bits above it (least-significant first) and the five zero bits of distance code 0 above those;
// bits 24..31 = the bit count. RFC 1951 3.2.5 / 3.2.6.
struct MatchTable {
  unsigned v[259];
  constexpr MatchTable() : v{} {
    constexpr int base[29] = {3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258};
    constexpr int extra[29] = {0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0};
    for (int m = 3; m <= 258; ++m) {
      int i = 28;
      while (base[i] > m) --i;
      const int sym = 257 + i;
      const int clen = sym < 280 ? 7 : 8;
      const unsigned code = sym < 280 ? (unsigned)(sym - 256) : 0xC0u + (unsigned)(sym - 280);
      unsigned rev = 0;
      for (int b = 0; b < clen; ++b) rev |= ((code >> b) & 1u) << (clen - 1 - b);
      v[m] = rev | ((unsigned)(m - base[i]) << clen) | ((unsigned)(clen + extra[i] + 5) << 24);
    }
  }
};
__constant__ MatchTable kMatch;
static_assert(MatchTable().v[258] == (kMatch258 | (kMatch258Bits << 24)), "length 258 is symbol 285 with no extra bits");
static_assert(MatchTable().v[3] >> 24 == 12 && MatchTable().v[257] >> 24 == 18, "7 + 0 + 5 and 8 + 5 + 5 bits");

__device__ __forceinline__ unsigned lit_bits(unsigned v) { return v < 144u ? 8u : 9u; }
// the literal's Huffman code (00110000 + v in 8 bits, 110010000 + v - 144 in 9), first bit in bit 0
__device__ __forceinline__ unsigned lit_code(unsigned v) { return v < 144u ? __brev(0x30u + v) >> 24 : __brev(0x190u + v - 144u) >> 23; }

// the bits of a run of n bytes v: the literal, (n - 1) / 258 full matches, and the rest as one match or as one or two literals
__device__ __forceinline__ unsigned run_bits(unsigned v, int n) {
  const int r = n - 1, q = r / 258, m = r - q * 258;
  return lit_bits(v) + (unsigned)q * kMatch258Bits + (m >= 3 ? kMatch.v[m] >> 24 : (unsigned)m * lit_bits(v));
}

__device__ __forceinline__ unsigned wave_sum_u32(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned wave_scan_u32(unsigned v, int lane) {   // inclusive
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned t = __shfl_up(v, o, 64);
    if (lane >= o) v += t;
  }
  return v;
}

// Appends codes at a bit position of a block: whole 32-bit words leave through atomicOr, never past word `limit` of the block.
struct BitWriter {
  unsigned* words;
  unsigned word, limit, fill;
  unsigned long long acc;
  __device__ __forceinline__ BitWriter(unsigned* w, unsigned bit, unsigned lim) : words(w), word(bit >> 5), limit(lim), fill(bit & 31u), acc(0) {}
  __device__ __forceinline__ void put(unsigned code, unsigned n) {          // n <= 18, fill < 32
    acc |= (unsigned long long)code << fill;
    fill += n;
    if (fill >= 32u) {
      if ((unsigned)acc && word < limit) atomicOr(words + word, (unsigned)acc);
      acc >>= 32;
      fill -= 32u;
      ++word;
    }
  }
  __device__ __forceinline__ void flush() {
    if ((unsigned)acc && word < limit) atomicOr(words + word, (unsigned)acc);
  }
};

// One wave walks one scanline, 64 bytes a step: position j of the scanline holds the filter byte 0
// (j = 0) or pixel j - 1; a lane whose byte starts a run (or that sits one past the scanline's end) closes the run before it, whose
// start is the nearest start below it in this step's ballot or, with none, the wave-uniform start carried from earlier steps.
// kEmit: the closing lane writes the run's tokens at bit0 + the bits of every run closed before it. Returns the scanline's bits;
// A / B: lane partials of its Adler sums (kEmit: not computed).
template <bool kEmit>
__device__ __forceinline__ unsigned walk_scanline(const unsigned char* __restrict__ row, int W, int lane, unsigned& A, unsigned& B,
                                                  unsigned* words, unsigned limit, unsigned bit0) {
  const int S = W + 1;
  int open = 0;
  unsigned last = 0, done = 0, mine = 0;
  for (int base = 0; base <= S; base += 64) {
    const int j = base + lane;
    const unsigned b = (j > 0 && j < S) ? row[j - 1] : 0u;
    unsigned pb = __shfl_up(b, 1, 64);
    if (lane == 0) pb = last;
    const bool start = j <= S && (j == 0 || j == S || b != pb);
    const unsigned long long mask = __ballot(start);
    unsigned cost = 0;
    int n = 0;
    if (start && j > 0) {
      const unsigned long long lower = mask & ((1ull << lane) - 1ull);
      n = j - (lower ? base + 63 - __clzll((long long)lower) : open);
      cost = run_bits(pb, n);
    }
    if constexpr (kEmit) {
      if (__ballot(cost != 0u)) {
        const unsigned incl = wave_scan_u32(cost, lane);
        if (cost) {
          BitWriter w(words, bit0 + done + incl - cost, limit);
          const unsigned lc = lit_code(pb), lb = lit_bits(pb);
          const int r = n - 1, q = r / 258, m = r - q * 258;
          w.put(lc, lb);
          for (int k = 0; k < q; ++k) w.put(kMatch258, kMatch258Bits);
          if (m >= 3) {
            const unsigned t = kMatch.v[m];
            w.put(t & 0xffffffu, t >> 24);
          } else {
            for (int k = 0; k < m; ++k) w.put(lc, lb);
          }
          w.flush();
        }
        done += __shfl(incl, 63, 64);
      }
    } else {
      mine += cost;
      if (j < S) {
        A += b;
        B += (unsigned)(S - j) * b;
      }
    }
    if (mask) open = base + 63 - __clzll((long long)mask);
    last = __shfl(b, 63, 64);
  }
  return kEmit ? done : wave_sum_u32(mine);
}

// workspace: three u32 arrays of n_planes * maxH entries (scanline y of plane p at p * maxH + y): the scanline's bits (after the
// plane pass: its bit offset in the block), A_y, and its Adler s2 term ((H - 1 - y) S A_y + B_y) mod 65521
__global__ __launch_bounds__(64 * kRowWaves) void png_measure_rows(const Plane* __restrict__ planes, int maxH, unsigned* __restrict__ bits,
                                                                  unsigned* __restrict__ rowA, unsigned* __restrict__ rowT) {
  const int p = blockIdx.y, lane = threadIdx.x & 63;
  const int y = blockIdx.x * kRowWaves + (threadIdx.x >> 6);
  const Plane pl = planes[p];
  if (y >= pl.H) return;
  unsigned A = 0, B = 0;
  const unsigned n = walk_scanline<false>(pl.plane + (size_t)y * pl.W, pl.W, lane, A, B, nullptr, 0u, 0u);
  A = wave_sum_u32(A);
  B = wave_sum_u32(B);
  if (lane == 0) {
    const size_t i = (size_t)p * maxH + y;
    const unsigned long long above = (unsigned long long)(pl.H - 1 - y) * (unsigned)(pl.W + 1) % kAdler;
    bits[i] = n;
    rowA[i] = A;
    rowT[i] = (unsigned)((above * (A % kAdler) + B) % kAdler);
  }
}

// one wave per plane: scanline bits -> bit offsets (in place), the block's byte length and the Adler-32
__global__ __launch_bounds__(64) void png_measure_planes(const Plane* __restrict__ planes, int maxH, unsigned* __restrict__ bits,
                                                        const unsigned* __restrict__ rowA, const unsigned* __restrict__ rowT,
                                                        unsigned* __restrict__ table) {
  const int p = blockIdx.x, lane = threadIdx.x;
  const int H = planes[p].H, S = planes[p].W + 1;
  unsigned carry = 3;                                     // BFINAL, BTYPE
  unsigned long long sA = 0, sT = 0;
  for (int base = 0; base < H; base += 64) {
    const int y = base + lane;
    const size_t i = (size_t)p * maxH + y;
    const unsigned c = y < H ? bits[i] : 0u;
    const unsigned incl = wave_scan_u32(c, lane);
    if (y < H) {
      bits[i] = carry + incl - c;
      sA += rowA[i];
      sT += rowT[i];
    }
    carry += __shfl(incl, 63, 64);
  }
  sA = wave_sum_u64(sA);
  sT = wave_sum_u64(sT);
  if (lane == 0) {
    const unsigned s1 = (unsigned)((1ull + sA) % kAdler);
    const unsigned s2 = (unsigned)(((unsigned long long)H * S + sT) % kAdler);
    table[4 * p + 1] = (carry + 7u + 7u) >> 3;            // end-of-block is seven zero bits, then zero bits up to a byte
    table[4 * p + 2] = s2 << 16 | s1;
    table[4 * p + 3] = 0u;
  }
}

// one wave: the planes' blocks back to back, each on a 4-byte boundary
__global__ __launch_bounds__(64) void png_measure_offsets(int n_planes, unsigned* __restrict__ table) {
  const int lane = threadIdx.x;
  unsigned carry = 0;
  for (int base = 0; base < n_planes; base += 64) {
    const int p = base + lane;
    const unsigned c = p < n_planes ? (table[4 * p + 1] + 3u) & ~3u : 0u;
    const unsigned incl = wave_scan_u32(c, lane);
    if (p < n_planes) table[4 * p] = carry + incl - c;
    carry += __shfl(incl, 63, 64);
  }
}

__global__ __launch_bounds__(64 * kRowWaves) void png_emit_rows(const Plane* __restrict__ planes, int maxH, const unsigned* __restrict__ bits,
                                                               const unsigned* __restrict__ table, unsigned char* __restrict__ out) {
  const int p = blockIdx.y, lane = threadIdx.x & 63;
  const int y = blockIdx.x * kRowWaves + (threadIdx.x >> 6);
  const Plane pl = planes[p];
  if (y >= pl.H) return;
  unsigned* words = reinterpret_cast<unsigned*>(out + table[4 * p]);
  const unsigned limit = (table[4 * p + 1] + 3u) >> 2;
  if (y == 0 && lane == 0) atomicOr(words, 3u);           // BFINAL = 1, BTYPE = 01 (least-significant bit first)
  unsigned A = 0, B = 0;
  walk_scanline<true>(pl.plane + (size_t)y * pl.W, pl.W, lane, A, B, words, limit, bits[(size_t)p * maxH + y]);
}

inline unsigned long block_bound(const Plane& pl) { return (10ul + 9ul * (unsigned long)(pl.W + 1) * (unsigned long)pl.H + 7ul) / 8ul; }

// the checks every call makes on its host table, and the tallest plane
int plan(const Plane* pl, int n_planes, int& maxH) {
  if (!pl || n_planes < 1 || n_planes > kMaxPlanes) return HAFF_ERR_BAD_ARG;
  unsigned long worst = 0;
  maxH = 0;
  for (int i = 0; i < n_planes; ++i) {
    if (!pl[i].plane || pl[i].H < 1 || pl[i].W < 1) return HAFF_ERR_BAD_ARG;
    if (pl[i].H > kMaxSide || pl[i].W > kMaxSide) return HAFF_ERR_UNSUPPORTED;
    worst += (block_bound(pl[i]) + 3ul) & ~3ul;
    maxH = pl[i].H > maxH ? pl[i].H : maxH;
  }
  return worst < (unsigned long)kMaxBytes ? HAFF_OK : HAFF_ERR_UNSUPPORTED;
}
inline long workspace_bytes_of(int n_planes, int maxH) { return 3L * 4L * n_planes * maxH; }

}  // namespace

extern "C" int haff_png_workspace(const haff_png_plane* planes_host, int n_planes, long* bytes_out) {
  if (!bytes_out) return HAFF_ERR_BAD_ARG;
  int maxH;
  const int rc = plan(planes_host, n_planes, maxH);
  if (rc != HAFF_OK) return rc;
  *bytes_out = workspace_bytes_of(n_planes, maxH);
  return HAFF_OK;
}

extern "C" int haff_png_measure(const haff_png_plane* planes_host, const haff_png_plane* planes_dev, int n_planes, void* workspace,
                                long workspace_bytes, unsigned* table, void* stream) {
  if (!planes_dev || !workspace || !table || !haff_aligned(workspace) || !haff_aligned(table)) return HAFF_ERR_BAD_ARG;
  int maxH;
  const int rc = plan(planes_host, n_planes, maxH);
  if (rc != HAFF_OK) return rc;
  if (workspace_bytes < workspace_bytes_of(n_planes, maxH)) return HAFF_ERR_BAD_ARG;
  const size_t rows = (size_t)n_planes * maxH;
  unsigned* bits = static_cast<unsigned*>(workspace);
  hipStream_t s = haff_stream(stream);
  png_measure_rows<<<dim3((maxH + kRowWaves - 1) / kRowWaves, n_planes), 64 * kRowWaves, 0, s>>>(planes_dev, maxH, bits, bits + rows, bits + 2 * rows);
  png_measure_planes<<<n_planes, 64, 0, s>>>(planes_dev, maxH, bits, bits + rows, bits + 2 * rows, table);
  png_measure_offsets<<<1, 64, 0, s>>>(n_planes, table);
  return haff_check_launch();
}

extern "C" int haff_png_emit(const haff_png_plane* planes_host, const haff_png_plane* planes_dev, int n_planes, const void* workspace,
                             long workspace_bytes, const unsigned* table_host, const unsigned* table_dev, unsigned char* out,
                             long out_bytes, void* stream) {
  if (!planes_dev || !workspace || !table_host || !table_dev || !out) return HAFF_ERR_BAD_ARG;
  if (!haff_aligned(workspace) || !haff_aligned(table_host, 4) || !haff_aligned(table_dev) || !haff_aligned(out, 4)) return HAFF_ERR_BAD_ARG;
  int maxH;
  const int rc = plan(planes_host, n_planes, maxH);
  if (rc != HAFF_OK) return rc;
  if (workspace_bytes < workspace_bytes_of(n_planes, maxH)) return HAFF_ERR_BAD_ARG;
  unsigned long need = 0;
  for (int i = 0; i < n_planes; ++i) {
    const unsigned long off = table_host[4 * i], len = table_host[4 * i + 1];
    if (off != need || len < 1 || len > block_bound(planes_host[i])) return HAFF_ERR_BAD_ARG;
    need += (len + 3ul) & ~3ul;
  }
  if (out_bytes < 0 || (unsigned long)out_bytes < need) return HAFF_ERR_BAD_ARG;
  hipStream_t s = haff_stream(stream);
  if (hipMemsetAsync(out, 0, need, s) != hipSuccess) return HAFF_ERR_LAUNCH;
  png_emit_rows<<<dim3((maxH + kRowWaves - 1) / kRowWaves, n_planes), 64 * kRowWaves, 0, s>>>(
      planes_dev, maxH, static_cast<const unsigned*>(workspace), table_dev, out);
  return haff_check_launch();
}
