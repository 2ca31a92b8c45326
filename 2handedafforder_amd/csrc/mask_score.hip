// Benchmark scoring on the device (ActAffordance/scripts/evaluation/calculate_iou.py:117-337 as evaluation.py restates it, and the
// validation metrics of 2Haff/train_ds.py:625-796): the comparison and the counting that used to leave HBM as PNGs or full planes.
//
//   haff_score_masks : one launch scores a batch of frames. Per frame (ScoreFrame, a 128-byte descriptor the host uploads): the two
//                      hands' fp32 logit planes [Hs][Ws] as evaluate() returns them, the frame's taxonomy probabilities, the two
//                      uint8 ground-truth planes and the two uint8 object planes [Hb][Wb], an optional uint8 output [T][Hb][Wb].
//                      For T <= 8 logit thresholds it adds up counts[frame][t] = {intersection, union, predicted area, ground-truth
//                      area} of the two-hand unions, and writes the predicted union (0/1) when asked.
//
// Per target pixel, hand and threshold: `cv2.resize` (bilinear on half-pixel centres) of the 0/255 plane `logit > th`, then `> 0`,
// decided in integers. Along each axis num = max((2o+1) n_in - n_out, 0), i0 = min(num / 2n_out, n_in-1), i1 = min(i0+1, n_in-1),
// w1 = num mod 2n_out (0 when i1 == i0), w0 = 2n_out - w1; S = sum over the four taps of wy wx [logit > th] (<= 4 Hb Wb <= 2^26);
// the resampled byte is round-half-even(255 S / (4 Hb Wb)), so the pixel is on iff 510 S > 4 Hb Wb (64-bit). Equal sizes give
// w1 = 0 on both axes: the identity. Comparisons are strict, so a NaN logit is off. Each hand is resampled alone, ANDed with
// `obj > 0` when it has an object plane, then the hands are ORed: the reference's order. The gate is inference.py's: argmax of
// the flattened taxonomy vector (first maximum, as gate_threshold_kernel), index 1 blanks the left hand, index 0 the right one.
//
// Grid (blocks per frame, frames), 256 threads, 4 consecutive target pixels per thread and iteration (one 4-B load of each uint8
// plane, one 4-B store per threshold where the address allows; bytes otherwise). The 256 KB source planes stay in L2; the
// target-side bytes are the traffic. Counts: ballot + popcount per wave into wave-uniform registers, one LDS slot per wave, one
// integer atomicAdd per counter and workgroup. Integer sums do not depend on arrival order: repeat runs are bitwise equal.
//
//   overlays (calculate_iou.py:43-95, create_overlay): a frame whose descriptor has vis = k draws through ScoreVis record k - 1
//   behind the frame table. A third launch, grid (blocks, records), 256 threads, 4 consecutive pixels of one frame row per thread:
//   the frame pixel's target pixel through the nearest-index tables, the hands' bits there by the SAME device functions the scoring
//   kernel counts with (taxonomy_gate, axis_taps, tap_sums, the 510 S rule, obj > 0) at the one threshold that is drawn, the
//   ground-truth bits, then two unfused fp32 blends with round-half-even and saturation in between: cv2.addWeighted twice on uint8.
//   12 bytes per canvas and thread, as three words where the canvas row allows; no atomics, no workspace.
#include "haff_common.h"

namespace {

constexpr int kMaxSide = 4096;      // (2o+1) n_in < 2^26 and S <= 4 Hb Wb <= 2^26: 32-bit taps and sums
constexpr int kMaxTh = 8;
constexpr int kMaxTax = 1024;       // taxonomy values read by one thread per workgroup
constexpr int kQuadsPerThread = 4;  // grid sizing: iterations of the widest frame's threads
constexpr int kMaxBlocks = 256;     // per frame; the rest is grid-strided

struct ScoreFrame {                 // == haff_score_frame (include/haff_hip.h)
  const float* logit[2];            // left, right: [Hs][Ws] or null (hand missing)
  const float* tax;                 // n_tax probabilities or null (gated by the caller)
  const unsigned char* gt[2];       // [Hb][Wb] or null (counts as empty)
  const unsigned char* obj[2];      // [Hb][Wb] or null (no AND)
  unsigned char* out;               // [T][Hb][Wb] or null
  int Hs, Ws, Hb, Wb, n_tax;
  int gt_hw[2][2], obj_hw[2][2];    // the planes' own shapes, checked on the host against (Hb, Wb)
  int vis;                          // 0, or 1 + the index of the frame's ScoreVis behind the frame table
  int pad[2];
};
static_assert(sizeof(ScoreFrame) == 128, "descriptor layout");
HAFF_SAME_SIZE(ScoreFrame, haff_score_frame);
HAFF_SAME_FIELD(ScoreFrame, logit, haff_score_frame, logit);
HAFF_SAME_FIELD(ScoreFrame, tax, haff_score_frame, taxonomy);
HAFF_SAME_FIELD(ScoreFrame, gt, haff_score_frame, gt);
HAFF_SAME_FIELD(ScoreFrame, obj, haff_score_frame, obj);
HAFF_SAME_FIELD(ScoreFrame, out, haff_score_frame, out);
HAFF_SAME_FIELD(ScoreFrame, Hs, haff_score_frame, Hs);
HAFF_SAME_FIELD(ScoreFrame, Ws, haff_score_frame, Ws);
HAFF_SAME_FIELD(ScoreFrame, Hb, haff_score_frame, Hb);
HAFF_SAME_FIELD(ScoreFrame, Wb, haff_score_frame, Wb);
HAFF_SAME_FIELD(ScoreFrame, n_tax, haff_score_frame, n_tax);
HAFF_SAME_FIELD(ScoreFrame, gt_hw, haff_score_frame, gt_hw);
HAFF_SAME_FIELD(ScoreFrame, obj_hw, haff_score_frame, obj_hw);
HAFF_SAME_FIELD(ScoreFrame, vis, haff_score_frame, vis);
HAFF_SAME_FIELD(ScoreFrame, pad, haff_score_frame, pad);

struct ScoreVis {                   // == haff_score_vis (include/haff_hip.h)
  const unsigned char* rgb;         // [Hf][Wf][3]
  const int* row;                   // [Hf] -> target row, or null with col: the identity
  const int* col;                   // [Wf] -> target column
  unsigned char* out[2];            // benchmark, prediction overlay; null = not drawn
  long stride[2];                   // bytes per canvas row
  int Hf, Wf, t;
  float alpha[2], beta[2], gamma;
  int color[2][3];
  int pad[4];
};
static_assert(sizeof(ScoreVis) == sizeof(ScoreFrame), "the vis records continue the frame table");
HAFF_SAME_SIZE(ScoreVis, haff_score_vis);
HAFF_SAME_FIELD(ScoreVis, rgb, haff_score_vis, rgb);
HAFF_SAME_FIELD(ScoreVis, row, haff_score_vis, row);
HAFF_SAME_FIELD(ScoreVis, col, haff_score_vis, col);
HAFF_SAME_FIELD(ScoreVis, out, haff_score_vis, out);
HAFF_SAME_FIELD(ScoreVis, stride, haff_score_vis, stride);
HAFF_SAME_FIELD(ScoreVis, Hf, haff_score_vis, Hf);
HAFF_SAME_FIELD(ScoreVis, Wf, haff_score_vis, Wf);
HAFF_SAME_FIELD(ScoreVis, t, haff_score_vis, t);
HAFF_SAME_FIELD(ScoreVis, alpha, haff_score_vis, alpha);
HAFF_SAME_FIELD(ScoreVis, beta, haff_score_vis, beta);
HAFF_SAME_FIELD(ScoreVis, gamma, haff_score_vis, gamma);
HAFF_SAME_FIELD(ScoreVis, color, haff_score_vis, color);
HAFF_SAME_FIELD(ScoreVis, pad, haff_score_vis, pad);

struct ScoreTh { float v[kMaxTh]; };

struct Taps { int i0, i1; unsigned w0, w1; };

__device__ __forceinline__ Taps axis_taps(int o, int n_in, int n_out) {
  int num = (2 * o + 1) * n_in - n_out;
  num = num < 0 ? 0 : num;
  const int den = 2 * n_out;
  Taps t;
  t.i0 = num / den;
  t.i0 = t.i0 > n_in - 1 ? n_in - 1 : t.i0;
  t.i1 = t.i0 + 1 > n_in - 1 ? n_in - 1 : t.i0 + 1;
  t.w1 = t.i1 == t.i0 ? 0u : (unsigned)(num % den);
  t.w0 = (unsigned)den - t.w1;
  return t;
}

// argmax of the frame's taxonomy vector, first maximum by strict > (a NaN never wins); -1 without one: both hands open
__device__ __forceinline__ int taxonomy_gate(const ScoreFrame& f) {
  int best = -1;
  if (f.tax) {
    best = 0;
    float bv = f.tax[0];
    for (int c = 1; c < f.n_tax; ++c) {
      const float v = f.tax[c];
      if (v > bv) { bv = v; best = c; }
    }
  }
  return best;
}

// S[t] += wy wx over the taps whose logit is above threshold t, for the first n_th of NT thresholds
template <int NT>
__device__ __forceinline__ void tap_sums(const float* src, int Ws, const Taps& ty, const Taps& tx, const float (&th)[NT], int n_th,
                                         unsigned (&S)[NT]) {
#pragma unroll
  for (int tap = 0; tap < 4; ++tap) {
    const unsigned w = ((tap & 2) ? ty.w1 : ty.w0) * ((tap & 1) ? tx.w1 : tx.w0);
    if (w == 0) continue;   // the clamped edge and the equal-size identity read one tap
    const float v = src[(long)((tap & 2) ? ty.i1 : ty.i0) * Ws + ((tap & 1) ? tx.i1 : tx.i0)];
#pragma unroll
    for (int t = 0; t < NT; ++t)
      if (t < n_th && v > th[t]) S[t] += w;
  }
}

// the resampled byte round-half-even(255 S / half) is above 0
__device__ __forceinline__ bool coverage_on(unsigned S, unsigned long long half) { return 510ull * S > half; }

// 4 bytes at p + b as one word when the address allows, the bytes below `total` otherwise
__device__ __forceinline__ unsigned load_quad(const unsigned char* p, long b, long total) {
  if (b + 4 <= total && (reinterpret_cast<uintptr_t>(p + b) & 3) == 0) return *reinterpret_cast<const unsigned*>(p + b);
  unsigned m = 0;
  for (int k = 0; k < 4 && b + k < total; ++k) m |= (unsigned)p[b + k] << (8 * k);
  return m;
}

// bit k <- byte k of m is non-zero
__device__ __forceinline__ unsigned nonzero_bits(unsigned m) {
  return ((m & 0xffu) ? 1u : 0u) | ((m & 0xff00u) ? 2u : 0u) | ((m & 0xff0000u) ? 4u : 0u) | ((m & 0xff000000u) ? 8u : 0u);
}

__global__ void score_zero_kernel(unsigned* counts, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) counts[i] = 0u;
}

__global__ __launch_bounds__(256) void score_masks_kernel(const ScoreFrame* frames, ScoreTh th, int n_th, unsigned* counts) {
  __shared__ int gate;
  __shared__ unsigned red[4][kMaxTh][4];
  const ScoreFrame f = frames[blockIdx.y];
  const long total = (long)f.Hb * f.Wb;
  const long n4 = (total + 3) >> 2;
  if ((long)blockIdx.x * 256 >= n4) return;   // a smaller frame of the batch: the whole workgroup leaves, before any barrier
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  if (tid == 0) gate = taxonomy_gate(f);
  __syncthreads();
  const int best = gate;
  const bool open[2] = {f.logit[0] != nullptr && best != 1, f.logit[1] != nullptr && best != 0};
  const unsigned long long half = 4ull * (unsigned long long)f.Hb * (unsigned long long)f.Wb;

  unsigned acc[kMaxTh][3] = {};   // wave-uniform: intersection, union, predicted area per threshold
  unsigned acc_gt = 0;

  // every lane of a wave runs every iteration (the ballots see the full wave); a lane past the end contributes zeros
  for (long base = (long)blockIdx.x * 256 + wave * 64; base < n4; base += (long)gridDim.x * 256) {
    const long i = base + lane;
    const bool live = i < n4;
    const long b = i << 2;
    unsigned gbits = 0, pm[kMaxTh] = {};
    if (live) {
      unsigned g = 0;
      if (f.gt[0]) g |= nonzero_bits(load_quad(f.gt[0], b, total));
      if (f.gt[1]) g |= nonzero_bits(load_quad(f.gt[1], b, total));
      const unsigned inside = b + 4 <= total ? 0xfu : (1u << (int)(total - b)) - 1u;
      gbits = g & inside;
      const int y_first = (int)(b / f.Wb), x_first = (int)(b % f.Wb);
      for (int h = 0; h < 2; ++h) {
        if (!open[h]) continue;
        unsigned ob = inside;
        if (f.obj[h]) ob &= nonzero_bits(load_quad(f.obj[h], b, total));
        if (!ob) continue;
        const float* src = f.logit[h];
        int y = y_first, x = x_first;
        Taps ty = axis_taps(y, f.Hs, f.Hb);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          if ((ob >> k) & 1u) {
            const Taps tx = axis_taps(x, f.Ws, f.Wb);
            unsigned S[kMaxTh] = {};
            tap_sums(src, f.Ws, ty, tx, th.v, n_th, S);
#pragma unroll
            for (int t = 0; t < kMaxTh; ++t)
              if (t < n_th && coverage_on(S[t], half)) pm[t] |= 1u << k;
          }
          if (++x == f.Wb) {
            x = 0;
            ++y;
            if (k < 3 && y < f.Hb) ty = axis_taps(y, f.Hs, f.Hb);
          }
        }
      }
      if (f.out) {
#pragma unroll
        for (int t = 0; t < kMaxTh; ++t) {
          if (t >= n_th) continue;
          unsigned char* o = f.out + (long)t * total + b;
          const unsigned w = (pm[t] & 1u) | ((pm[t] & 2u) << 7) | ((pm[t] & 4u) << 14) | ((pm[t] & 8u) << 21);
          if (b + 4 <= total && (reinterpret_cast<uintptr_t>(o) & 3) == 0) {
            *reinterpret_cast<unsigned*>(o) = w;
          } else {
            for (int k = 0; k < 4 && b + k < total; ++k) o[k] = (unsigned char)(w >> (8 * k));
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const bool g = (gbits >> k) & 1u;
      acc_gt += (unsigned)__popcll(__ballot(g));
#pragma unroll
      for (int t = 0; t < kMaxTh; ++t) {
        if (t >= n_th) continue;
        const bool p = (pm[t] >> k) & 1u;
        acc[t][0] += (unsigned)__popcll(__ballot(p && g));
        acc[t][1] += (unsigned)__popcll(__ballot(p || g));
        acc[t][2] += (unsigned)__popcll(__ballot(p));
      }
    }
  }

  if (lane == 0) {
#pragma unroll
    for (int t = 0; t < kMaxTh; ++t) {
      red[wave][t][0] = acc[t][0];
      red[wave][t][1] = acc[t][1];
      red[wave][t][2] = acc[t][2];
      red[wave][t][3] = acc_gt;
    }
  }
  __syncthreads();
  if (tid < 4 * n_th) {
    const int t = tid >> 2, c = tid & 3;
    const unsigned s = red[0][t][c] + red[1][t][c] + red[2][t][c] + red[3][t][c];
    if (s) atomicAdd(counts + ((long)blockIdx.y * n_th + t) * 4 + c, s);
  }
}

// cv2.addWeighted on uint8, one channel: a * alpha + b * beta + gamma in fp32, unfused, then cvRound (half to even) and saturation
__device__ __forceinline__ float add_weighted(float a, float alpha, float b, float beta, float gamma) {
  float pa = __fmul_rn(a, alpha), pb = __fmul_rn(b, beta);
  asm volatile("" : "+v"(pa), "+v"(pb));   // the build contracts across statements (-ffp-contract=fast): keep both products' roundings
  const float v = rintf(__fadd_rn(__fadd_rn(pa, pb), gamma));
  return v < 0.f ? 0.f : (v > 255.f ? 255.f : v);   // a NaN weight lands on 255 by the compares, never outside a byte
}

constexpr int kVisPixels = 4;       // consecutive pixels of one frame row per thread: 12 bytes, three words
constexpr int kVisMaxBlocks = 1024; // per record; the rest is grid-strided

// Record blockIdx.y of the ScoreVis table behind the n_frames frame descriptors. The frame that names it is found by a scan of the
// descriptors' vis fields (the host refuses a record named twice, so at most one thread finds one).
__global__ __launch_bounds__(256) void score_vis_kernel(const ScoreFrame* frames, int n_frames, ScoreTh th) {
  __shared__ int owner, gate;
  const int tid = threadIdx.x;
  if (tid == 0) owner = -1;
  __syncthreads();
  for (int i = tid; i < n_frames; i += 256)
    if (frames[i].vis == (int)blockIdx.y + 1) owner = i;
  __syncthreads();
  if (owner < 0) return;            // a record no frame names: nothing to draw (uniform over the workgroup)
  const ScoreFrame f = frames[owner];
  const ScoreVis v = reinterpret_cast<const ScoreVis*>(frames + n_frames)[blockIdx.y];
  const int qw = (v.Wf + kVisPixels - 1) / kVisPixels;   // threads per frame row
  const long items = (long)v.Hf * qw;
  if ((long)blockIdx.x * 256 >= items) return;            // a smaller frame of the batch, before the gate's barrier
  if (tid == 0) gate = taxonomy_gate(f);
  __syncthreads();
  const int best = gate;
  const bool open[2] = {f.logit[0] != nullptr && best != 1, f.logit[1] != nullptr && best != 0};
  const unsigned long long half = 4ull * (unsigned long long)f.Hb * (unsigned long long)f.Wb;
  float th1[1] = {0.f};
#pragma unroll
  for (int k = 0; k < kMaxTh; ++k)
    if (k == v.t) th1[0] = th.v[k];

  for (long item = (long)blockIdx.x * 256 + tid; item < items; item += (long)gridDim.x * 256) {
    const int y = (int)(item / qw), x0 = (int)(item % qw) * kVisPixels;
    const int n = v.Wf - x0 < kVisPixels ? v.Wf - x0 : kVisPixels;
    int yb = v.row ? v.row[y] : y;
    yb = yb < 0 ? 0 : (yb > f.Hb - 1 ? f.Hb - 1 : yb);
    const Taps ty = axis_taps(yb, f.Hs, f.Hb);

    // the frame's 12 bytes: three words where the address allows
    const unsigned char* src = v.rgb + ((long)y * v.Wf + x0) * 3;
    unsigned char px[3 * kVisPixels] = {};
    if (n == kVisPixels && (reinterpret_cast<uintptr_t>(src) & 3) == 0) {
#pragma unroll
      for (int w = 0; w < 3; ++w) {
        const unsigned m = reinterpret_cast<const unsigned*>(src)[w];
#pragma unroll
        for (int b = 0; b < 4; ++b) px[4 * w + b] = (unsigned char)(m >> (8 * b));
      }
    } else {
#pragma unroll
      for (int b = 0; b < 3 * kVisPixels; ++b)
        if (b < 3 * n) px[b] = src[b];
    }

    // layer bits per pixel: bit 0 / 1 = left / right ground truth, bit 2 / 3 = left / right prediction
    unsigned bits[kVisPixels] = {};
#pragma unroll
    for (int k = 0; k < kVisPixels; ++k) {
      if (k >= n) continue;
      int xb = v.col ? v.col[x0 + k] : x0 + k;
      xb = xb < 0 ? 0 : (xb > f.Wb - 1 ? f.Wb - 1 : xb);
      const long at = (long)yb * f.Wb + xb;
      const Taps tx = axis_taps(xb, f.Ws, f.Wb);
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        if (f.gt[h] && f.gt[h][at] > 0) bits[k] |= 1u << h;
        if (!open[h]) continue;
        if (f.obj[h] && !(f.obj[h][at] > 0)) continue;
        unsigned S[1] = {0u};
        tap_sums(f.logit[h], f.Ws, ty, tx, th1, 1, S);
        if (coverage_on(S[0], half)) bits[k] |= 4u << h;
      }
    }

#pragma unroll
    for (int c = 0; c < 2; ++c) {         // canvas 0: benchmark layers, canvas 1: prediction layers
      if (!v.out[c]) continue;
      unsigned char res[3 * kVisPixels];
#pragma unroll
      for (int k = 0; k < kVisPixels; ++k) {
        const bool L = (bits[k] >> (2 * c)) & 1u, R = (bits[k] >> (2 * c + 1)) & 1u;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) {
          const float t1 = add_weighted((float)px[3 * k + ch], v.alpha[0], L ? (float)v.color[0][ch] : 0.f, v.beta[0], v.gamma);
          const float t2 = add_weighted(t1, v.alpha[1], R ? (float)v.color[1][ch] : 0.f, v.beta[1], v.gamma);
          res[3 * k + ch] = (unsigned char)t2;
        }
      }
      unsigned char* dst = v.out[c] + (long)y * v.stride[c] + (long)x0 * 3;
      if (n == kVisPixels && (reinterpret_cast<uintptr_t>(dst) & 3) == 0) {
#pragma unroll
        for (int w = 0; w < 3; ++w)
          reinterpret_cast<unsigned*>(dst)[w] = (unsigned)res[4 * w] | ((unsigned)res[4 * w + 1] << 8) | ((unsigned)res[4 * w + 2] << 16) |
                                                ((unsigned)res[4 * w + 3] << 24);
      } else {
#pragma unroll
        for (int b = 0; b < 3 * kVisPixels; ++b)
          if (b < 3 * n) dst[b] = res[b];
      }
    }
  }
}

}  // namespace

extern "C" int haff_score_masks(const void* frames_host, const void* frames_dev, int n_frames, const float* thresholds_host,
                                int n_th, void* counts, void* stream) {
  if (!frames_host || !frames_dev || !thresholds_host || !counts || n_frames <= 0 || n_frames > 65535) return HAFF_ERR_BAD_ARG;
  if (n_th < 1 || n_th > kMaxTh) return HAFF_ERR_BAD_ARG;
  if (!haff_aligned(frames_host, 8) || !haff_aligned(frames_dev, 8) || !haff_aligned(counts, 4)) return HAFF_ERR_BAD_ARG;
  const ScoreFrame* fr = static_cast<const ScoreFrame*>(frames_host);
  long blocks = 1, vis_blocks = 1;
  int n_vis = 0;                                  // overlay records behind the table: the largest vis of the batch
  unsigned long long vis_seen[1024] = {};         // one bit per record (n_frames <= 65535): a record draws for one frame
  for (int i = 0; i < n_frames; ++i) {
    const ScoreFrame& f = fr[i];
    if (f.Hs <= 0 || f.Ws <= 0 || f.Hb <= 0 || f.Wb <= 0) return HAFF_ERR_BAD_ARG;
    if (f.Hs > kMaxSide || f.Ws > kMaxSide || f.Hb > kMaxSide || f.Wb > kMaxSide) return HAFF_ERR_UNSUPPORTED;
    if (f.tax && (f.n_tax < 1 || f.n_tax > kMaxTax)) return HAFF_ERR_BAD_ARG;
    if (!haff_aligned(f.logit[0], 4) || !haff_aligned(f.logit[1], 4) || !haff_aligned(f.tax, 4)) return HAFF_ERR_BAD_ARG;
    for (int h = 0; h < 2; ++h) {
      if (f.gt[h] && (f.gt_hw[h][0] != f.Hb || f.gt_hw[h][1] != f.Wb)) return HAFF_ERR_BAD_ARG;
      if (f.obj[h] && (f.obj_hw[h][0] != f.Hb || f.obj_hw[h][1] != f.Wb)) return HAFF_ERR_BAD_ARG;
    }
    const long n4 = ((long)f.Hb * f.Wb + 3) >> 2;
    long g = (n4 + 256L * kQuadsPerThread - 1) / (256L * kQuadsPerThread);
    g = g > kMaxBlocks ? kMaxBlocks : g;
    blocks = g > blocks ? g : blocks;
    if (f.vis == 0) continue;
    // the frame's overlay record, behind the frame table
    if (f.vis < 1 || f.vis > n_frames) return HAFF_ERR_BAD_ARG;
    if (vis_seen[(f.vis - 1) >> 6] >> ((f.vis - 1) & 63) & 1ull) return HAFF_ERR_BAD_ARG;
    vis_seen[(f.vis - 1) >> 6] |= 1ull << ((f.vis - 1) & 63);
    const ScoreVis& v = reinterpret_cast<const ScoreVis*>(fr + n_frames)[f.vis - 1];
    if (v.Hf < 1 || v.Wf < 1) return HAFF_ERR_BAD_ARG;
    if (v.Hf > kMaxSide || v.Wf > kMaxSide) return HAFF_ERR_UNSUPPORTED;
    if (!v.rgb || (!v.out[0] && !v.out[1])) return HAFF_ERR_BAD_ARG;
    if ((v.row == nullptr) != (v.col == nullptr)) return HAFF_ERR_BAD_ARG;
    if (!v.row && (v.Hf != f.Hb || v.Wf != f.Wb)) return HAFF_ERR_BAD_ARG;
    if (!haff_aligned(v.row, 4) || !haff_aligned(v.col, 4)) return HAFF_ERR_BAD_ARG;
    if (v.t < 0 || v.t >= n_th) return HAFF_ERR_BAD_ARG;
    for (int c = 0; c < 2; ++c)
      if (v.out[c] && v.stride[c] < 3L * v.Wf) return HAFF_ERR_BAD_ARG;
    const long items = (long)v.Hf * ((v.Wf + kVisPixels - 1) / kVisPixels);
    long vg = (items + 255) / 256;
    vg = vg > kVisMaxBlocks ? kVisMaxBlocks : vg;
    vis_blocks = vg > vis_blocks ? vg : vis_blocks;
    n_vis = f.vis > n_vis ? f.vis : n_vis;
  }
  ScoreTh th{};
  for (int t = 0; t < n_th; ++t) th.v[t] = thresholds_host[t];
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const long n_counts = (long)n_frames * n_th * 4;
  hipLaunchKernelGGL(score_zero_kernel, dim3((unsigned)((n_counts + 255) / 256)), dim3(256), 0, s, (unsigned*)counts, n_counts);
  hipLaunchKernelGGL(score_masks_kernel, dim3((unsigned)blocks, (unsigned)n_frames), dim3(256), 0, s,
                     static_cast<const ScoreFrame*>(frames_dev), th, n_th, (unsigned*)counts);
  if (n_vis)
    hipLaunchKernelGGL(score_vis_kernel, dim3((unsigned)vis_blocks, (unsigned)n_vis), dim3(256), 0, s,
                       static_cast<const ScoreFrame*>(frames_dev), n_frames, th);
  return haff_check_launch();
}
