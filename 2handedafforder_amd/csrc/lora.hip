// Rank-r adapter kernels of the LoRA fine-tune path (reference: peft LoraConfig on q_proj / v_proj, 2Haff/train_ds.py:192-230;
// the adapted projections feed LlamaAttention's rotate-half RoPE, model/llava/model/language_model/llava_llama.py:76-101).
//
//   forward    q = rope(x.Wq^T + s.(x.Aq^T).Bq^T),  k = rope(x.Wk^T),  v = x.Wv^T + s.(x.Av^T).Bv^T
//
// The frozen product x.[Wq;Wk;Wv]^T is the tile GEMM's; everything a rank-8 update adds is HBM-bound row traffic, and the
// generic route (four N = 8 / K = 8 products on the 128 x 128 tile, scale, add, two RoPE passes, and in backward three
// transposes per dW plus the zero-fill / copy / add chain of autograd's slice adjoints) cost ~0.9 ms per Llama layer and
// step — 14 % of the configs[3] step. Here:
//   * t^T = A2.x^T [16][M] (A2 = [Aq; Av]) is ONE weight-streaming launch of gemm_bf16.hip with the roles swapped (the
//     activation rows are the streamed operand);
//   * lora_qkv_rope_fwd_kernel reads q|k|v once, adds the rank-r update with one 75 %-empty MFMA per 16 x 16 tile (k = the
//     adapter index: the matrix pipe is idle on this path anyway), rotates q and k, writes the three attention operands;
//   * lora_qkv_rope_bwd_kernel assembles d(qkv) = [rope^T dq | rope^T dk | dv] in one pass (no slice adjoints);
//   * dt^T = B^T.dq^T is again the swapped weight-streaming product; lora_dx_kernel adds s.keep.(dt.A2) into the d(x) the
//     frozen product's adjoint wrote; lora_tn_kernel is the one contraction over ROWS (dA = dt^T.x, dB = dq^T.t): rank rows
//     in SGPRs, the big operand streamed once, per-row-block partials summed in index order (no atomics, deterministic).
// LoRA on the other projections (--lora_target_modules): the q|k|v kernel with a third (k) adapter, t^T [24][M]; lora_out_kernel
// adds an adapted Linear's update into the frozen product's rows (o_proj, down_proj, residual already in); lora_gu_swiglu_kernel
// adds the gate and up updates into the interleaved gate|up product and applies SwiGLU in the same pass.
// bf16 or f16 storage (every kernel is one template, F16 = the fp16 fine-tune's instance: the *_f16 entry points), fp32
// arithmetic, head dim 128, rank <= 8 per adapter.
#include "haff_common.h"

namespace {

constexpr int HD = 128;   // head dim (Llama 7B / 13B)

__device__ __forceinline__ bf16x8 zero_frag() { return bf16x8{0, 0, 0, 0, 0, 0, 0, 0}; }

// the 16 x 32 operand tile of t (rows = activation rows row0.., k = adapter rank index 0..8na-1, the rest empty) out of
// t^T [8na][ldt]: na = 2 adapters (q, v) or 3 (q, v, k)
__device__ __forceinline__ bf16x8 load_t_frag(const bf16_t* tT, long ldt, long row, int fh, int na) {
  bf16x8 f = zero_frag();
  if (fh < na) {
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = (short)tT[(long)(8 * fh + i) * ldt + row];
  }
  return f;
}

struct LoraFwdArgs {
  const bf16_t* qkv; long ld_qkv;
  const bf16_t* tT; long ldt;
  const bf16_t *Bq, *Bv; int ldb;
  const float* cs;
  bf16_t *qo, *ko, *vo; long ldo;
  long M; int H, T; float scale;
  const bf16_t* Bk;   // NA = 3 (haff_lora_qkv3_rope_fwd): the k adapter's B, its ranks at t^T rows 16-23
};

// one wave = one head x 16-row tiles. The head's 128 columns are four groups of 32 (groups 2, 3 = the rotate-half partners of
// groups 0, 1); a group takes TWO MFMAs whose column operands are loaded in a permuted order (MFMA h, operand row i = column
// 8 * (i / 4) + 4 * h + i % 4), so that lane (fr, fh) ends up with row fr, columns 8fh .. 8fh+7 of the group: 16-byte
// loads and stores, 64 contiguous bytes per row and instruction (the natural operand order leaves 4 columns per lane:
// 8-byte accesses in 32-byte runs, which held this kernel at 2.4 TB/s)
template <bool F16, int NA>
__global__ __launch_bounds__(256, 3) void lora_qkv_rope_fwd_kernel(LoraFwdArgs p) {
  using E = h16<F16>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, fh = lane >> 4;
  const int head = blockIdx.x;
  const long n_rt = (p.M + 15) / 16;
  bf16x8 bq[4][2], bv[4][2], bk[4][2];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const long col = (long)head * HD + 32 * g + 8 * (fr >> 2) + 4 * h + (fr & 3);
      bq[g][h] = fh == 0 ? *reinterpret_cast<const bf16x8*>(p.Bq + col * p.ldb) : zero_frag();
      bv[g][h] = fh == 1 ? *reinterpret_cast<const bf16x8*>(p.Bv + col * p.ldb) : zero_frag();
      bk[g][h] = (NA == 3 && fh == 2) ? *reinterpret_cast<const bf16x8*>(p.Bk + col * p.ldb) : zero_frag();
    }
  for (long rt = (long)blockIdx.y * 4 + wave; rt < n_rt; rt += (long)gridDim.y * 4) {
    const long row = rt * 16 + fr;
    const bool valid = row < p.M;
    const long rc = valid ? row : p.M - 1;
    const int pos = (int)(rc % p.T);
    const bf16x8 tt = load_t_frag(p.tT, p.ldt, rc, fh, NA);
    const bf16_t* src = p.qkv + rc * p.ld_qkv + (long)head * HD + 8 * fh;
    bf16_t* q_o = p.qo + rc * p.ldo + (long)head * HD + 8 * fh;
    bf16_t* k_o = p.ko + rc * p.ldo + (long)head * HD + 8 * fh;
    bf16_t* v_o = p.vo + rc * p.ldo + (long)head * HD + 8 * fh;
    const float* csr = p.cs + (long)pos * HD + 8 * fh;
#pragma unroll
    for (int g = 0; g < 2; ++g) {   // column group g and its rotate-half partner g + 2
      float qa[8], qb[8], ka[8], kb[8], va[8], vb[8], co[8], si[8];
      load8h<F16>(src + 32 * g, qa); load8h<F16>(src + 64 + 32 * g, qb);
      load8h<F16>(src + p.H + 32 * g, ka); load8h<F16>(src + p.H + 64 + 32 * g, kb);
      load8h<F16>(src + 2 * (long)p.H + 32 * g, va); load8h<F16>(src + 2 * (long)p.H + 64 + 32 * g, vb);
      load8(csr + 32 * g, co); load8(csr + 64 + 32 * g, si);
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      f32x4 dq0[2], dq1[2], dv0[2], dv1[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        dq0[h] = E::mfma16(bq[g][h], tt, z);
        dq1[h] = E::mfma16(bq[g + 2][h], tt, z);
        dv0[h] = E::mfma16(bv[g][h], tt, z);
        dv1[h] = E::mfma16(bv[g + 2][h], tt, z);
      }
      if constexpr (NA == 3) {   // the k adapter's update lands on k BEFORE its rotation, as q's does
        f32x4 dk0[2], dk1[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          dk0[h] = E::mfma16(bk[g][h], tt, z);
          dk1[h] = E::mfma16(bk[g + 2][h], tt, z);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          ka[e] += p.scale * dk0[e >> 2][e & 3];
          kb[e] += p.scale * dk1[e >> 2][e & 3];
        }
      }
      float q1[8], q2[8], k1[8], k2[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float ql = qa[e] + p.scale * dq0[e >> 2][e & 3], qh = qb[e] + p.scale * dq1[e >> 2][e & 3];
        q1[e] = ql * co[e] - qh * si[e];
        q2[e] = qh * co[e] + ql * si[e];
        k1[e] = ka[e] * co[e] - kb[e] * si[e];
        k2[e] = kb[e] * co[e] + ka[e] * si[e];
        va[e] += p.scale * dv0[e >> 2][e & 3];
        vb[e] += p.scale * dv1[e >> 2][e & 3];
      }
      if (valid) {
        store8h<F16>(q_o + 32 * g, q1); store8h<F16>(q_o + 64 + 32 * g, q2);
        store8h<F16>(k_o + 32 * g, k1); store8h<F16>(k_o + 64 + 32 * g, k2);
        store8h<F16>(v_o + 32 * g, va); store8h<F16>(v_o + 64 + 32 * g, vb);
      }
    }
  }
}

// d(qkv) [M][3H] = [rope^T dq | rope^T dk | dv]: thread = (row, head, 8 low columns + their partners)
template <bool F16>
__global__ __launch_bounds__(256) void lora_qkv_rope_bwd_kernel(const bf16_t* dq, const bf16_t* dk, const bf16_t* dv, long ld_in,
                                                              const float* cs, bf16_t* dqkv, long ld_out, long M, int H, int T) {
  const int nh = H / HD;
  const long total = M * nh * 8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int ch = (int)(i & 7);
    const int head = (int)((i >> 3) % nh);
    const long row = (i >> 3) / nh;
    const int pos = (int)(row % T);
    const long col = (long)head * HD + 8 * ch;
    float co[8], si[8];
    load8(cs + (long)pos * HD + 8 * ch, co);
    load8(cs + (long)pos * HD + 64 + 8 * ch, si);
    float a[8], b[8], x1[8], x2[8];
    load8h<F16>(dq + row * ld_in + col, a);
    load8h<F16>(dq + row * ld_in + col + 64, b);
#pragma unroll
    for (int e = 0; e < 8; ++e) { x1[e] = a[e] * co[e] + b[e] * si[e]; x2[e] = b[e] * co[e] - a[e] * si[e]; }
    store8h<F16>(dqkv + row * ld_out + col, x1);
    store8h<F16>(dqkv + row * ld_out + col + 64, x2);
    load8h<F16>(dk + row * ld_in + col, a);
    load8h<F16>(dk + row * ld_in + col + 64, b);
#pragma unroll
    for (int e = 0; e < 8; ++e) { x1[e] = a[e] * co[e] + b[e] * si[e]; x2[e] = b[e] * co[e] - a[e] * si[e]; }
    store8h<F16>(dqkv + row * ld_out + H + col, x1);
    store8h<F16>(dqkv + row * ld_out + H + col + 64, x2);
    *reinterpret_cast<uint4*>(dqkv + row * ld_out + 2 * (long)H + col) = *reinterpret_cast<const uint4*>(dv + row * ld_in + col);
    *reinterpret_cast<uint4*>(dqkv + row * ld_out + 2 * (long)H + col + 64) = *reinterpret_cast<const uint4*>(dv + row * ld_in + col + 64);
  }
}

// dx[row][col] (+)= scale * keep[row][col] * sum_j dt[row][j] * A2[j][col]: wave = 128 columns x 16-row tiles
struct LoraDxArgs {
  const bf16_t* dtT; long ldt;
  const bf16_t* A2; long lda;
  const bf16_t* keep; long ldk;
  bf16_t* dx; long ldx;
  long M; int K; int accumulate; float scale;
  const bf16_t* keep_v;   // two masks (haff_lora_dx2): `keep` gates the q adapter's ranks (rows 0-7 of A2), keep_v the v adapter's (8-15)
  const bf16_t* keep_k;   // three masks (haff_lora_dx3): keep_k gates the k adapter's ranks (rows 16-23 of A3)
  int na;                 // adapters (8 rank rows each) in dt^T / A: 2, or 3 (haff_lora_dx3)
};
template <bool F16>
__global__ __launch_bounds__(256) void lora_dx_kernel(LoraDxArgs p) {   // column operands permuted as in the forward kernel
  using E = h16<F16>;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int fr = lane & 15, fh = lane >> 4;
  const long c0 = (long)blockIdx.x * 128;
  const long n_rt = (p.M + 15) / 16;
  bf16x8 af[4][2];
#pragma unroll
  for (int g = 0; g < 4; ++g)
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      af[g][h] = zero_frag();
      if (fh < p.na) {
        const long col = c0 + 32 * g + 8 * (fr >> 2) + 4 * h + (fr & 3);
#pragma unroll
        for (int i = 0; i < 8; ++i) af[g][h][i] = (short)p.A2[(long)(8 * fh + i) * p.lda + col];
      }
    }
  for (long rt = (long)blockIdx.y * 4 + wave; rt < n_rt; rt += (long)gridDim.y * 4) {
    const long row = rt * 16 + fr;
    const bool valid = row < p.M;
    const long rc = valid ? row : p.M - 1;
    const bf16x8 tt = load_t_frag(p.dtT, p.ldt, rc, fh, p.na);
    bf16_t* dst = p.dx + rc * p.ldx + c0 + 8 * fh;
    const bf16_t* kpr = p.keep ? p.keep + rc * p.ldk + c0 + 8 * fh : nullptr;
    const bf16_t* kvr = p.keep_v ? p.keep_v + rc * p.ldk + c0 + 8 * fh : nullptr;
    const bf16_t* kkr = p.keep_k ? p.keep_k + rc * p.ldk + c0 + 8 * fh : nullptr;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float old[8], kp[8], kv[8], kk[8];
      if (p.accumulate) load8h<F16>(dst + 32 * g, old);
      if (kpr) load8h<F16>(kpr + 32 * g, kp);
      if (kvr) load8h<F16>(kvr + 32 * g, kv);
      if (kkr) load8h<F16>(kkr + 32 * g, kk);
      const f32x4 z = {0.f, 0.f, 0.f, 0.f};
      f32x4 d[2];
      float v[8];
      if (kvr) {   // (wave-uniform) two masks: the q adapter's ranks sit in the fh = 0 lanes of the A fragment, the v adapter's in fh = 1
        const bf16x8 zf = zero_frag();
        f32x4 dv[2], dk[2];
        d[0] = E::mfma16(fh == 0 ? af[g][0] : zf, tt, z);
        d[1] = E::mfma16(fh == 0 ? af[g][1] : zf, tt, z);
        dv[0] = E::mfma16(fh == 1 ? af[g][0] : zf, tt, z);
        dv[1] = E::mfma16(fh == 1 ? af[g][1] : zf, tt, z);
        if (kkr) {   // (wave-uniform) the third mask: the k adapter's ranks in the fh = 2 lanes
          dk[0] = E::mfma16(fh == 2 ? af[g][0] : zf, tt, z);
          dk[1] = E::mfma16(fh == 2 ? af[g][1] : zf, tt, z);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          v[e] = p.scale * (d[e >> 2][e & 3] * kp[e] + dv[e >> 2][e & 3] * kv[e]);
          if (kkr) v[e] += p.scale * (dk[e >> 2][e & 3] * kk[e]);
          if (p.accumulate) v[e] += old[e];
        }
      } else {
        d[0] = E::mfma16(af[g][0], tt, z);
        d[1] = E::mfma16(af[g][1], tt, z);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          v[e] = p.scale * d[e >> 2][e & 3];
          if (kpr) v[e] *= kp[e];
          if (p.accumulate) v[e] += old[e];
        }
      }
      if (valid) store8h<F16>(dst + 32 * g, v);
    }
  }
}

// part[rb][j][n] = sum over the row block's rows m of sT[j][m] * big[m][n]: workgroup = 128 columns (2 per lane) x one row
// block; its 4 waves take 8-row groups in turn (the R x 8 rank values of a group are wave-uniform: scalar loads), and meet in
// LDS in wave order
template <int R, bool F16>
__global__ __launch_bounds__(256) void lora_tn_kernel(const bf16_t* sT, long lds, const bf16_t* big, long ldb, long M, int N,
                                                      int rows_per_block, float* part) {
  using E = h16<F16>;
  __shared__ float red[4][R][128];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const long col = (long)blockIdx.x * 128 + 2 * lane;
  const long colc = col < N ? col : 0;   // N % 2 == 0 (checked by the launcher); columns past N are computed on column 0 and dropped
  const long r_lo = (long)blockIdx.y * rows_per_block;
  long r_hi = r_lo + rows_per_block;
  if (r_hi > M) r_hi = M;
  float acc[R][2];
#pragma unroll
  for (int j = 0; j < R; ++j) acc[j][0] = acc[j][1] = 0.f;
  // 16 rows per step (r_lo % 64 == 0, lds % 8 == 0 and lds >= roundup(M, 16): 32-B aligned rank rows), the next step's 16
  // loads of the big operand in flight while this step's 2 * 16 * R FMAs run: a wave has only a handful of steps, and
  // with one memory round trip per step the launch ran at a quarter of the HBM rate
  auto load_rows = [&](long m0, unsigned (&bw)[16]) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {   // rows past the block re-read its last row (their rank value is forced to 0 below)
      const long m = m0 + i < r_hi ? m0 + i : r_hi - 1;
      bw[i] = *reinterpret_cast<const unsigned*>(big + m * ldb + colc);
    }
  };
  unsigned bw[16], nx[16];
  long m0 = r_lo + 16 * wave;
  if (m0 < r_hi) load_rows(m0, bw);
  for (; m0 < r_hi; m0 += 64) {
    const bool more = m0 + 64 < r_hi;
    if (more) load_rows(m0 + 64, nx);
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const uint4 s0 = *reinterpret_cast<const uint4*>(sT + (long)j * lds + m0);
      const uint4 s1 = *reinterpret_cast<const uint4*>(sT + (long)j * lds + m0 + 8);
      const unsigned sw[8] = {s0.x, s0.y, s0.z, s0.w, s1.x, s1.y, s1.z, s1.w};
#pragma unroll
      for (int i = 0; i < 16; ++i) {
        const float h = (i & 1) ? E::hi(sw[i >> 1]) : E::lo(sw[i >> 1]);
        const float sv = (m0 + i < r_hi) ? h : 0.f;
        acc[j][0] = fmaf(sv, E::lo(bw[i]), acc[j][0]);
        acc[j][1] = fmaf(sv, E::hi(bw[i]), acc[j][1]);
      }
    }
    if (more) {
#pragma unroll
      for (int i = 0; i < 16; ++i) bw[i] = nx[i];
    }
  }
#pragma unroll
  for (int j = 0; j < R; ++j) {
    red[wave][j][2 * lane] = acc[j][0];
    red[wave][j][2 * lane + 1] = acc[j][1];
  }
  __syncthreads();
  float* dst = part + (long)blockIdx.y * R * N;
  for (int e = threadIdx.x; e < R * 128; e += 256) {
    const int j = e >> 7, c = e & 127;
    const long n = (long)blockIdx.x * 128 + c;
    if (n < N) dst[(long)j * N + n] = ((red[0][j][c] + red[1][j][c]) + red[2][j][c]) + red[3][j][c];
  }
}

// out = scale * sum over row blocks (index order) of part[rb][j][n]; rows j < j_valid only; [j][n] or transposed [n][j]
template <typename TO>
__global__ void lora_tn_reduce_kernel(const float* part, int nrb, int R, int N, TO* out, long ldo, int transposed, int j_valid,
                                      float scale) {
  const long total = (long)j_valid * N;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int j = (int)(i / N);
    const long n = i - (long)j * N;
    float s = 0.f;
    for (int rb = 0; rb < nrb; ++rb) s += part[((long)rb * R + j) * N + n];
    s *= scale;
    elem<TO>::st(transposed ? out + n * ldo + j : out + (long)j * ldo + n, s);
  }
}

// An adapted Linear's rank-8 update added into the frozen product's output, which already holds its residual epilogue
// (o_proj, down_proj):  y[m][n] += scale * sum_j t[m][j] * B[n][j],  t^T [8][ldt] (ldt % 4 == 0, columns past M finite).
// Thread = 4 rows x 8 columns: B's 8 x 8 block stays in registers, the 4 rows' rank values come in as one 8-byte load per rank
// (the same address in every lane of a wave whose lanes walk the columns), y is read and written once with 16-byte accesses.
template <bool F16>
__global__ __launch_bounds__(256) void lora_out_kernel(const bf16_t* tT, long ldt, const bf16_t* B, bf16_t* y, long ldy, long M, int N,
                                                       float scale) {
  using E = h16<F16>;
  const int n8 = N >> 3;
  const long total = (M + 3) / 4 * n8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long m0 = (i / n8) * 4;
    const long c = (i - (m0 / 4) * n8) * 8;
    float b[8][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) load8h<F16>(B + (c + e) * 8, b[e]);
    float t[4][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint2 w = *reinterpret_cast<const uint2*>(tT + (long)j * ldt + m0);
      t[0][j] = E::lo(w.x); t[1][j] = E::hi(w.x); t[2][j] = E::lo(w.y); t[3][j] = E::hi(w.y);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (m0 + r >= M) break;
      bf16_t* dst = y + (m0 + r) * ldy + c;
      float o[8];
      load8h<F16>(dst, o);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float acc = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc = fmaf(t[r][j], b[e][j], acc);
        o[e] += scale * acc;
      }
      store8h<F16>(dst, o);
    }
  }
}

// gate | up with SwiGLU: gu [M][2F] in the interleaved [gate x16 | up x16] column layout of the frozen product. The gate
// adapter's ranks are t^T rows 0-7 (Bg [F][8]), the up adapter's rows 8-15 (Bu [F][8]); output f's gate column takes Bg row f,
// its up column Bu row f (a block-structured B over the interleaved rows: each column sees one adapter's 8 ranks only).
//   gu[m][.] += scale * update (IN PLACE: the SwiGLU adjoint's operand),  y[m][f] = silu(g') * u'
// Thread = 4 rows x 8 outputs (8 gate + 8 up columns of one 16-column half group).
template <bool F16>
__global__ __launch_bounds__(256) void lora_gu_swiglu_kernel(const bf16_t* tT, long ldt, const bf16_t* Bg, const bf16_t* Bu, bf16_t* gu,
                                                             long ldg, bf16_t* y, long ldy, long M, int F, float scale) {
  using E = h16<F16>;
  const int f8 = F >> 3;
  const long total = (M + 3) / 4 * f8;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long m0 = (i / f8) * 4;
    const long f = (i - (m0 / 4) * f8) * 8;
    const long base = (f >> 4) * 32 + (f & 15);
    float bg[8][8], bu[8][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      load8h<F16>(Bg + (f + e) * 8, bg[e]);
      load8h<F16>(Bu + (f + e) * 8, bu[e]);
    }
    float tg[4][8], tu[4][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const uint2 w = *reinterpret_cast<const uint2*>(tT + (long)j * ldt + m0);
      const uint2 v = *reinterpret_cast<const uint2*>(tT + (long)(8 + j) * ldt + m0);
      tg[0][j] = E::lo(w.x); tg[1][j] = E::hi(w.x); tg[2][j] = E::lo(w.y); tg[3][j] = E::hi(w.y);
      tu[0][j] = E::lo(v.x); tu[1][j] = E::hi(v.x); tu[2][j] = E::lo(v.y); tu[3][j] = E::hi(v.y);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      if (m0 + r >= M) break;
      bf16_t* g_p = gu + (m0 + r) * ldg + base;
      float g[8], u[8], o[8];
      load8h<F16>(g_p, g);
      load8h<F16>(g_p + 16, u);
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float ag = 0.f, au = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          ag = fmaf(tg[r][j], bg[e][j], ag);
          au = fmaf(tu[r][j], bu[e][j], au);
        }
        g[e] += scale * ag;
        u[e] += scale * au;
      }
      store8h<F16>(g_p, g);
      store8h<F16>(g_p + 16, u);
      // silu of the values as STORED (rounded to 16 bits): the adjoint reads gu' back, so forward and backward see one g', u'
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float gs = E::to_f32(E::from_f32(g[e])), us = E::to_f32(E::from_f32(u[e]));
        o[e] = gs / (1.0f + expf(-gs)) * us;
      }
      store8h<F16>(y + (m0 + r) * ldy + f, o);
    }
  }
}

}  // namespace

// rows of the 2-D launches (x = gx column groups: heads, or 128-column groups): 16-row tiles, four per workgroup (one per wave),
// capped at ~2048 workgroups in all (8 per CU); the waves stride over the row tiles that are left
static unsigned lora_rows_grid(long M, int gx) {
  const long gy = ((M + 15) / 16 + 3) / 4, cap = (2048 + gx - 1) / gx;
  return (unsigned)(gy > cap ? cap : gy);
}

static void lora_fwd_args(LoraFwdArgs& p, const void* qkv, long ld_qkv, const void* tT, long ldt, const void* Bq, const void* Bv, const void* Bk,
                          int ldb, const float* cos_sin, void* q_out, void* k_out, void* v_out, long ldo, long M, int H, int T, float scale) {
  p.qkv = (const bf16_t*)qkv; p.ld_qkv = ld_qkv; p.tT = (const bf16_t*)tT; p.ldt = ldt;
  p.Bq = (const bf16_t*)Bq; p.Bv = (const bf16_t*)Bv; p.Bk = (const bf16_t*)Bk; p.ldb = ldb; p.cs = cos_sin;
  p.qo = (bf16_t*)q_out; p.ko = (bf16_t*)k_out; p.vo = (bf16_t*)v_out; p.ldo = ldo;
  p.M = M; p.H = H; p.T = T; p.scale = scale;
}

template <bool F16, int NA>
static int lora_qkv_rope_fwd_impl(const void* qkv, long ld_qkv, const void* tT, long ldt, const void* Bq, const void* Bv, const void* Bk,
                                  int ldb, const float* cos_sin, void* q_out, void* k_out, void* v_out, long ldo, long M, int H, int d,
                                  int T, float scale, void* stream) {
  if (M <= 0 || T <= 0 || H <= 0 || !qkv || !tT || !Bq || !Bv || !cos_sin || !q_out || !k_out || !v_out) return HAFF_ERR_BAD_ARG;
  if (NA == 3 && (!Bk || !haff_aligned(Bk))) return HAFF_ERR_BAD_ARG;
  if (d != HD || H % HD || ldb != 8) return HAFF_ERR_UNSUPPORTED;
  if (ld_qkv < 3L * H || ldo < H || ldt < M || (ld_qkv & 7) || (ldo & 7)) return HAFF_ERR_BAD_ARG;
  for (const void* x : {qkv, Bq, Bv, (const void*)cos_sin, (const void*)q_out, (const void*)k_out, (const void*)v_out})
    if (!haff_aligned(x)) return HAFF_ERR_BAD_ARG;
  LoraFwdArgs p;
  lora_fwd_args(p, qkv, ld_qkv, tT, ldt, Bq, Bv, Bk, ldb, cos_sin, q_out, k_out, v_out, ldo, M, H, T, scale);
  const int nh = H / HD;
  hipLaunchKernelGGL((lora_qkv_rope_fwd_kernel<F16, NA>), dim3(nh, lora_rows_grid(M, nh)), dim3(256), 0, haff_stream(stream), p);
  return haff_check_launch();
}

template <bool F16>
static int lora_qkv_rope_bwd_impl(const void* dq, const void* dk, const void* dv, long ld_in, const float* cos_sin, void* dqkv,
                                  long ld_out, long M, int H, int d, int T, void* stream) {
  if (M <= 0 || T <= 0 || H <= 0 || !dq || !dk || !dv || !cos_sin || !dqkv) return HAFF_ERR_BAD_ARG;
  if (d != HD || H % HD) return HAFF_ERR_UNSUPPORTED;
  if (ld_in < H || ld_out < 3L * H || (ld_in & 7) || (ld_out & 7)) return HAFF_ERR_BAD_ARG;
  if (!haff_aligned(dq) || !haff_aligned(dk) || !haff_aligned(dv) || !haff_aligned(cos_sin) || !haff_aligned(dqkv)) return HAFF_ERR_BAD_ARG;
  hipLaunchKernelGGL((lora_qkv_rope_bwd_kernel<F16>), dim3(haff_grid(M * (H / HD) * 8, 256, 16384)), dim3(256), 0, haff_stream(stream),
                     (const bf16_t*)dq, (const bf16_t*)dk, (const bf16_t*)dv, ld_in, cos_sin, (bf16_t*)dqkv, ld_out, M, H, T);
  return haff_check_launch();
}

// The dropout masks each dx entry point takes (its `masks` = how many it has parameters for): haff_lora_dx none or its one; haff_lora_dx2
// both; haff_lora_dx3 none, keep_q alone (one mask for every adapter) or all three. A parameter the entry point lacks arrives null.
static bool lora_dx_masks_ok(int masks, const void* keep_q, const void* keep_v, const void* keep_k) {
  if (masks == 2) return keep_q && keep_v;
  return (!keep_v && !keep_k) || (masks == 3 && keep_q && keep_v && keep_k);
}

static void lora_dx_args(LoraDxArgs& p, const void* dtT, long ldt, const void* A, long lda, const void* keep_q, const void* keep_v,
                         const void* keep_k, long ldk, void* dx, long ldx, int accumulate, long M, int K, float scale, int na) {
  p.dtT = (const bf16_t*)dtT; p.ldt = ldt; p.A2 = (const bf16_t*)A; p.lda = lda;
  p.keep = (const bf16_t*)keep_q; p.keep_v = (const bf16_t*)keep_v; p.keep_k = (const bf16_t*)keep_k; p.ldk = ldk;
  p.dx = (bf16_t*)dx; p.ldx = ldx; p.M = M; p.K = K; p.accumulate = accumulate; p.scale = scale; p.na = na;
}

// masks: the mask parameters of the entry point (1, 2 or 3, see lora_dx_masks_ok); na: the adapter slots of dt^T / A (2, or 3 for _dx3)
template <bool F16>
static int lora_dx_launch(int masks, int na, const void* dtT, long ldt, const void* A, long lda, const void* keep_q, const void* keep_v,
                          const void* keep_k, long ldk, void* dx, long ldx, int accumulate, long M, int K, float scale, void* stream) {
  if (M <= 0 || K <= 0 || !dtT || !A || !dx || !lora_dx_masks_ok(masks, keep_q, keep_v, keep_k)) return HAFF_ERR_BAD_ARG;
  if (!haff_aligned(keep_k)) return HAFF_ERR_BAD_ARG;   // judged BEFORE the K % 128 rule, keep_q / keep_v after it: recorded, kept as it is
  if (K % 128) return HAFF_ERR_UNSUPPORTED;
  if (ldt < M || lda < K || ldx < K || (ldx & 7) || (keep_q && (ldk < K || (ldk & 7)))) return HAFF_ERR_BAD_ARG;
  if (!haff_aligned(dx) || !haff_aligned(keep_q) || !haff_aligned(keep_v)) return HAFF_ERR_BAD_ARG;
  LoraDxArgs p;
  lora_dx_args(p, dtT, ldt, A, lda, keep_q, keep_v, keep_k, ldk, dx, ldx, accumulate, M, K, scale, na);
  const int gx = K / 128;
  hipLaunchKernelGGL((lora_dx_kernel<F16>), dim3(gx, lora_rows_grid(M, gx)), dim3(256), 0, haff_stream(stream), p);
  return haff_check_launch();
}

// rows per block of haff_lora_tn (multiple of 64): ~16 row blocks
static long lora_tn_rows_per_block(long M) {
  long rpb = ((M + 15) / 16 + 63) / 64 * 64;
  return rpb < 64 ? 64 : rpb;
}
static long lora_tn_ws(long M, int R, int N) {
  const long rpb = lora_tn_rows_per_block(M);
  return ((M + rpb - 1) / rpb) * (long)R * N;
}

template <bool F16>
static int lora_tn_impl(const void* sT, long lds, int R, const void* big, long ldb, long M, int N, float* workspace, long workspace_elems,
                        void* out, long ldo, int out_f32, int transposed, int j_valid, float scale, void* stream) {
  if (M <= 0 || N <= 0 || !sT || !big || !workspace || !out || j_valid <= 0 || j_valid > R) return HAFF_ERR_BAD_ARG;
  if (R != 8 && R != 16) return HAFF_ERR_UNSUPPORTED;
  if ((lds & 7) || lds < (M + 15) / 16 * 16 || !haff_aligned(sT) || (N & 1) || (ldb & 1) || ldb < N || !haff_aligned(big, 4))
    return HAFF_ERR_BAD_ARG;
  if (workspace_elems < lora_tn_ws(M, R, N)) return HAFF_ERR_BAD_ARG;
  if (ldo < (transposed ? j_valid : N)) return HAFF_ERR_BAD_ARG;
  const long rpb = lora_tn_rows_per_block(M);
  const int nrb = (int)((M + rpb - 1) / rpb);
  const dim3 g((N + 127) / 128, nrb), b(256);
  hipStream_t s = haff_stream(stream);
  HAFF_DISPATCH_BOOL(R == 8, R8, hipLaunchKernelGGL((lora_tn_kernel<R8 ? 8 : 16, F16>), g, b, 0, s, (const bf16_t*)sT, lds, (const bf16_t*)big, ldb, M, N,
                                                    (int)rpb, workspace));
  HAFF_DISPATCH_OUT16(out_f32, F16, hipLaunchKernelGGL((lora_tn_reduce_kernel<T>), dim3(haff_grid((long)j_valid * N, 256, 4096)), b, 0, s, workspace,
                                                        nrb, R, N, (T*)out, ldo, transposed, j_valid, scale));
  return haff_check_launch();
}

extern "C" int haff_lora_qkv_rope_fwd(const void* qkv, long ld_qkv, const void* tT, long ldt, const void* Bq, const void* Bv,
                                      int ldb, const float* cos_sin, void* q_out, void* k_out, void* v_out, long ldo, long M,
                                      int H, int d, int T, float scale, void* stream) {
  return lora_qkv_rope_fwd_impl<false, 2>(qkv, ld_qkv, tT, ldt, Bq, Bv, nullptr, ldb, cos_sin, q_out, k_out, v_out, ldo, M, H, d, T, scale,
                                          stream);
}

extern "C" int haff_lora_qkv_rope_bwd(const void* dq, const void* dk, const void* dv, long ld_in, const float* cos_sin, void* dqkv,
                                      long ld_out, long M, int H, int d, int T, void* stream) {
  return lora_qkv_rope_bwd_impl<false>(dq, dk, dv, ld_in, cos_sin, dqkv, ld_out, M, H, d, T, stream);
}

extern "C" int haff_lora_dx(const void* dtT, long ldt, const void* A2, long lda, const void* keep, long ldk, void* dx, long ldx,
                            int accumulate, long M, int K, float scale, void* stream) {
  return lora_dx_launch<false>(1, 2, dtT, ldt, A2, lda, keep, nullptr, nullptr, ldk, dx, ldx, accumulate, M, K, scale, stream);
}

// haff_lora_dx with TWO dropout masks (peft: one lora_dropout module per adapted Linear, 2Haff/train_ds.py:218-230):
//   dx (+)= scale * ( keep_q o (dt[0:8]^T . A2[0:8]) + keep_v o (dt[8:16]^T . A2[8:16]) ),   both masks bf16 [M][ldk] of values,
//   both required (lora_dx_masks_ok; haff_lora_dx3 below: no mask, keep_q alone for every adapter, or all three).
extern "C" int haff_lora_dx2(const void* dtT, long ldt, const void* A2, long lda, const void* keep_q, const void* keep_v, long ldk,
                             void* dx, long ldx, int accumulate, long M, int K, float scale, void* stream) {
  return lora_dx_launch<false>(2, 2, dtT, ldt, A2, lda, keep_q, keep_v, nullptr, ldk, dx, ldx, accumulate, M, K, scale, stream);
}

extern "C" int haff_lora_tn_workspace_elems(long M, int R, int N) {   // f32 values haff_lora_tn wants; < 0: does not fit an int
  const long n = (M > 0 && R > 0 && N > 0) ? lora_tn_ws(M, R, N) : -1;
  return n > 0x7fffffffL ? HAFF_ERR_UNSUPPORTED : (int)n;
}
extern "C" int haff_lora_tn(const void* sT, long lds, int R, const void* big, long ldb, long M, int N, float* workspace,
                            long workspace_elems, void* out, long ldo, int out_f32, int transposed, int j_valid, float scale,
                            void* stream) {
  return lora_tn_impl<false>(sT, lds, R, big, ldb, M, N, workspace, workspace_elems, out, ldo, out_f32, transposed, j_valid, scale, stream);
}

// ---- fp16 instances (fp16 fine-tuning): every 16-bit operand, mask and result IEEE binary16; same arguments and contracts ----
extern "C" int haff_lora_qkv_rope_fwd_f16(const void* qkv, long ld_qkv, const void* tT, long ldt, const void* Bq, const void* Bv,
                                          int ldb, const float* cos_sin, void* q_out, void* k_out, void* v_out, long ldo, long M,
                                          int H, int d, int T, float scale, void* stream) {
  return lora_qkv_rope_fwd_impl<true, 2>(qkv, ld_qkv, tT, ldt, Bq, Bv, nullptr, ldb, cos_sin, q_out, k_out, v_out, ldo, M, H, d, T, scale,
                                         stream);
}
extern "C" int haff_lora_qkv_rope_bwd_f16(const void* dq, const void* dk, const void* dv, long ld_in, const float* cos_sin, void* dqkv,
                                          long ld_out, long M, int H, int d, int T, void* stream) {
  return lora_qkv_rope_bwd_impl<true>(dq, dk, dv, ld_in, cos_sin, dqkv, ld_out, M, H, d, T, stream);
}
extern "C" int haff_lora_dx_f16(const void* dtT, long ldt, const void* A2, long lda, const void* keep, long ldk, void* dx, long ldx,
                                int accumulate, long M, int K, float scale, void* stream) {
  return lora_dx_launch<true>(1, 2, dtT, ldt, A2, lda, keep, nullptr, nullptr, ldk, dx, ldx, accumulate, M, K, scale, stream);
}
extern "C" int haff_lora_dx2_f16(const void* dtT, long ldt, const void* A2, long lda, const void* keep_q, const void* keep_v, long ldk,
                                 void* dx, long ldx, int accumulate, long M, int K, float scale, void* stream) {
  return lora_dx_launch<true>(2, 2, dtT, ldt, A2, lda, keep_q, keep_v, nullptr, ldk, dx, ldx, accumulate, M, K, scale, stream);
}
extern "C" int haff_lora_tn_f16(const void* sT, long lds, int R, const void* big, long ldb, long M, int N, float* workspace,
                                long workspace_elems, void* out, long ldo, int out_f32, int transposed, int j_valid, float scale,
                                void* stream) {
  return lora_tn_impl<true>(sT, lds, R, big, ldb, M, N, workspace, workspace_elems, out, ldo, out_f32, transposed, j_valid, scale, stream);
}

// ---- all-projection LoRA (--lora_target_modules): a k adapter in the fused q|k|v node, and the adapted o / down / gate|up ----

template <bool F16>
static int lora_out_impl(const void* tT, long ldt, const void* B, void* y, long ldy, long M, int N, float scale, void* stream) {
  if (M <= 0 || N <= 0 || !tT || !B || !y) return HAFF_ERR_BAD_ARG;
  if (N % 8) return HAFF_ERR_UNSUPPORTED;
  if (ldt < (M + 3) / 4 * 4 || (ldt & 3) || !haff_aligned(tT, 8) || ldy < N || (ldy & 7) || !haff_aligned(y) || !haff_aligned(B))
    return HAFF_ERR_BAD_ARG;
  hipLaunchKernelGGL((lora_out_kernel<F16>), dim3(haff_grid((M + 3) / 4 * (N / 8), 256, 8192)), dim3(256), 0, haff_stream(stream),
                     (const bf16_t*)tT, ldt, (const bf16_t*)B, (bf16_t*)y, ldy, M, N, scale);
  return haff_check_launch();
}

template <bool F16>
static int lora_gu_swiglu_impl(const void* tT, long ldt, const void* Bg, const void* Bu, void* gu, long ldg, void* y, long ldy, long M, int F,
                               float scale, void* stream) {
  if (M <= 0 || F <= 0 || !tT || !Bg || !Bu || !gu || !y) return HAFF_ERR_BAD_ARG;
  if (F % 16) return HAFF_ERR_UNSUPPORTED;
  if (ldt < (M + 3) / 4 * 4 || (ldt & 3) || !haff_aligned(tT, 8) || ldg < 2L * F || (ldg & 7) || ldy < F || (ldy & 7))
    return HAFF_ERR_BAD_ARG;
  if (!haff_aligned(Bg) || !haff_aligned(Bu) || !haff_aligned(gu) || !haff_aligned(y)) return HAFF_ERR_BAD_ARG;
  hipLaunchKernelGGL((lora_gu_swiglu_kernel<F16>), dim3(haff_grid((M + 3) / 4 * (F / 8), 256, 8192)), dim3(256), 0, haff_stream(stream),
                     (const bf16_t*)tT, ldt, (const bf16_t*)Bg, (const bf16_t*)Bu, (bf16_t*)gu, ldg, (bf16_t*)y, ldy, M, F, scale);
  return haff_check_launch();
}

extern "C" int haff_lora_qkv3_rope_fwd(const void* qkv, long ld_qkv, const void* tT, long ldt, const void* Bq, const void* Bv, const void* Bk,
                                       int ldb, const float* cos_sin, void* q_out, void* k_out, void* v_out, long ldo, long M, int H, int d,
                                       int T, float scale, void* stream) {
  return lora_qkv_rope_fwd_impl<false, 3>(qkv, ld_qkv, tT, ldt, Bq, Bv, Bk, ldb, cos_sin, q_out, k_out, v_out, ldo, M, H, d, T, scale, stream);
}
extern "C" int haff_lora_dx3(const void* dtT, long ldt, const void* A3, long lda, const void* keep_q, const void* keep_v, const void* keep_k,
                             long ldk, void* dx, long ldx, int accumulate, long M, int K, float scale, void* stream) {
  return lora_dx_launch<false>(3, 3, dtT, ldt, A3, lda, keep_q, keep_v, keep_k, ldk, dx, ldx, accumulate, M, K, scale, stream);
}
extern "C" int haff_lora_out(const void* tT, long ldt, const void* B, void* y, long ldy, long M, int N, float scale, void* stream) {
  return lora_out_impl<false>(tT, ldt, B, y, ldy, M, N, scale, stream);
}
extern "C" int haff_lora_gu_swiglu(const void* tT, long ldt, const void* Bg, const void* Bu, void* gu, long ldg, void* y, long ldy, long M,
                                   int F, float scale, void* stream) {
  return lora_gu_swiglu_impl<false>(tT, ldt, Bg, Bu, gu, ldg, y, ldy, M, F, scale, stream);
}
extern "C" int haff_lora_qkv3_rope_fwd_f16(const void* qkv, long ld_qkv, const void* tT, long ldt, const void* Bq, const void* Bv,
                                           const void* Bk, int ldb, const float* cos_sin, void* q_out, void* k_out, void* v_out, long ldo,
                                           long M, int H, int d, int T, float scale, void* stream) {
  return lora_qkv_rope_fwd_impl<true, 3>(qkv, ld_qkv, tT, ldt, Bq, Bv, Bk, ldb, cos_sin, q_out, k_out, v_out, ldo, M, H, d, T, scale, stream);
}
extern "C" int haff_lora_dx3_f16(const void* dtT, long ldt, const void* A3, long lda, const void* keep_q, const void* keep_v,
                                 const void* keep_k, long ldk, void* dx, long ldx, int accumulate, long M, int K, float scale, void* stream) {
  return lora_dx_launch<true>(3, 3, dtT, ldt, A3, lda, keep_q, keep_v, keep_k, ldk, dx, ldx, accumulate, M, K, scale, stream);
}
extern "C" int haff_lora_out_f16(const void* tT, long ldt, const void* B, void* y, long ldy, long M, int N, float scale, void* stream) {
  return lora_out_impl<true>(tT, ldt, B, y, ldy, M, N, scale, stream);
}
extern "C" int haff_lora_gu_swiglu_f16(const void* tT, long ldt, const void* Bg, const void* Bu, void* gu, long ldg, void* y, long ldy,
                                       long M, int F, float scale, void* stream) {
  return lora_gu_swiglu_impl<true>(tT, ldt, Bg, Bu, gu, ldg, y, ldy, M, F, scale, stream);
}
