/*
 * haff_hip.h — C-ABI of libhaff_hip.so, the MI355X (gfx950 / CDNA4) hot path of pearl-robot-lab/2HandedAfforder.
 *
 * The reference has no FFI / plugin boundary of its own: its per-frame path is Python
 * (`LISAForCausalLM.evaluate`, 2Haff/model/LISA.py:432-534) over torch + transformers. This library sits UNDER
 * that Python boundary: each entry point replaces the torch / transformers op(s) cited next to it, and is what a
 * maintainer binds with ctypes from the reference's own modules.
 *
 * Conventions
 *   - all pointers are caller-owned DEVICE pointers (HBM) unless marked "host"; no internal allocation; re-entrant;
 *     `stream` is a hipStream_t passed as void* (0 = null stream); kernels are only enqueued. No process-wide setting:
 *     the one piece of state the library keeps is haff_gemm_stream_cap's table, keyed by stream and guarded by a mutex
 *     (scheduling only, results never depend on it) — host threads that enqueue on different streams do not interact.
 *   - return value: 0 ok, -1 bad argument, -2 unsupported shape, -3 launch error. No exceptions cross the ABI.
 *   - dtype codes: 0 = bf16 (raw 16-bit payload), 1 = f32, 3 = f16 (IEEE binary16). bf16 = throughput mode (bf16 MFMA,
 *     fp32 accumulate, fp32 softmax/norm statistics); f32 = parity mode (every op in fp32, for the 1e-3 mask-logit criterion);
 *     f16 = the inference mode of the reference's `--precision fp16` (f16 MFMA, otherwise as bf16). Code 2 is the norms'
 *     "f32 x -> bf16 y". Entry points named *_bf16 take no dtype; those the fp16 path needs have *_f16 siblings with the
 *     same arguments and contracts (one kernel template, two instances). The data-movement entry points and
 *     haff_upscale_mask return -1 for a code (or an in/out pair) they have no kernel for: none falls through to f32.
 *   - strides/leading dimensions are in ELEMENTS.
 *   - activation codes: 0 none, 1 GELU(erf), 2 quick-GELU (x*sigmoid(1.702x)), 3 ReLU, 4 SiLU.
 */
#ifndef HAFF_HIP_H
#define HAFF_HIP_H

/* return codes of every entry point */
#define HAFF_OK 0
#define HAFF_ERR_BAD_ARG (-1)
#define HAFF_ERR_UNSUPPORTED (-2)
#define HAFF_ERR_LAUNCH (-3)

#ifdef __cplusplus
extern "C" {
#endif

/* ---- GEMM with fused epilogue: C[M,N] = act(A[M,K] . W[N,K]^T + bias) + resid -------------------------------
 * Replaces every nn.Linear / 1x1 conv / patchify conv on the path: SAM qkv/proj/MLP (image_encoder.py:223-224,258;
 * common.py:13-26), CLIP & Llama linears (transformers, reached from clip_encoder.py:53-56 / llava_llama.py:93-105),
 * mm_projector (llava_arch.py:35), text_hidden_fcs (LISA.py:95-101), SAM decoder linears (transformer.py:206-209),
 * first ConvTranspose2d of the upscaler (mask_decoder.py:55-57) as a per-pixel GEMM.
 * row_map (int32[M], may be null): output AND residual row = row_map[m]; negative = row dropped (fuses
 * window_unpartition, image_encoder.py:291-318). swiglu != 0: W rows interleaved in 16-row groups
 * [gate x16 | up x16], output width N/2 = silu(gate)*up (LlamaMLP). out_f32: C (and resid) are f32.
 * Requirements: K % 8 == 0, lda % 8 == 0, ldw % 8 == 0, A and W 16-byte aligned. */
int haff_gemm_bf16(const void* A, long lda, const void* W, long ldw, void* C, long ldc, const float* bias,
                   const void* resid, long ldr, const int* row_map, int M, int N, int K, int act, int out_f32,
                   int swiglu, void* stream);
/* same, with an explicit tile choice for measurements: 0 auto, 1 = 128x128, 2 = 256x256, 3 = 192x256 workgroup tile */
int haff_gemm_bf16_cfg(const void* A, long lda, const void* W, long ldw, void* C, long ldc, const float* bias,
                       const void* resid, long ldr, const int* row_map, int M, int N, int K, int act, int out_f32,
                       int swiglu, int tile_cfg, void* stream);
/* haff_gemm_bf16 with a caller-provided DEVICE workspace (16-B aligned; 16 * M * N bytes are used when it applies): for
 * 33..64-row products on weights of <= 8192 rows (the decode-step o_proj / down_proj of llava_llama.py:93-102 at batch 64)
 * the weight-streaming kernel splits K over workgroups, fp32 partial tiles go through the workspace and are summed in a
 * fixed order (deterministic). NULL workspace, or a shape with no useful split: identical to haff_gemm_bf16. */
int haff_gemm_bf16_ws(const void* A, long lda, const void* W, long ldw, void* C, long ldc, const float* bias,
                      const void* resid, long ldr, const int* row_map, int M, int N, int K, int act, int out_f32,
                      int swiglu, void* workspace, long workspace_bytes, void* stream);
/* fp16 instances of haff_gemm_bf16 / _cfg / _ws: A, W and a 16-bit C / resid are f16 (v_mfma_f32_16x16x32_f16, fp32 accumulate) */
int haff_gemm_f16(const void* A, long lda, const void* W, long ldw, void* C, long ldc, const float* bias,
                  const void* resid, long ldr, const int* row_map, int M, int N, int K, int act, int out_f32,
                  int swiglu, void* stream);
int haff_gemm_f16_cfg(const void* A, long lda, const void* W, long ldw, void* C, long ldc, const float* bias,
                      const void* resid, long ldr, const int* row_map, int M, int N, int K, int act, int out_f32,
                      int swiglu, int tile_cfg, void* stream);
int haff_gemm_f16_ws(const void* A, long lda, const void* W, long ldw, void* C, long ldc, const float* bias,
                     const void* resid, long ldr, const int* row_map, int M, int N, int K, int act, int out_f32,
                     int swiglu, void* workspace, long workspace_bytes, void* stream);
/* fp16 instances of the fused products below (_rms, _gather, _qkv_rope, _rowstats, _ln, _heads): same arguments and contracts, f16
 * operands / 16-bit outputs / caches / residuals; statistics, biases and RoPE tables stay f32 */
int haff_gemm_f16_rms(const void* A, long lda, const void* W, long ldw, void* C, long ldc, const float* bias,
                      const void* resid, long ldr, int M, int N, int K, int act, int out_f32, int swiglu,
                      const float* ssq_in, int ssq_n, float eps, float* ssq_out, int* n_parts_out, void* stream);
int haff_gemm_f16_gather(const void* A, long lda, const int* a_map, long a_rows, const void* W, long ldw, void* C,
                         long ldc, const float* bias, const void* resid, long ldr, const int* row_map, int M, int N,
                         int K, int act, int out_f32, int swiglu, void* stream);
int haff_gemm_f16_qkv_rope(const void* A, long lda, const void* Wp, long ldw, void* q_out, long ldq, void* kcache,
                           void* vcache, const float* cos_sin, int B, int T, int Tmax, int pos0, int H, int d, int K,
                           void* stream);
int haff_gemm_f16_rowstats(const void* A, long lda, const int* a_map, long a_rows, const void* W, long ldw, void* C,
                           long ldc, const float* bias, const void* resid, long ldr, int M, int N, int K,
                           float* stat_out, void* stream);
int haff_gemm_f16_ln(const void* A, long lda, const void* W, long ldw, void* C, long ldc, const float* bias,
                     const void* resid, long ldr, const int* row_map, const float* ln_stats, const float* ln_colsum,
                     int M, int N, int K, int act, int out_f32, int swiglu, void* stream);
int haff_gemm_f16_heads(const void* A, long lda, const void* W, long ldw, void* C, const float* bias, const int* row_map,
                        const float* ln_stats, const float* ln_colsum, int M, int N, int K, int d, int heads, long part_stride,
                        long head_stride, void* stream);
/* NF4 language-model weights of the fp16 mode (load_in_4bit; csrc/gemm_nf4.hip, format restated in quant.py). Row-local storage:
 * packed uint8 [N][K/2] (code of W[n][k] in byte k/2, even k in the high nibble), absmax f32 [N][K/64] = the DEQUANTISED block
 * absmax; K % 64 == 0. A weight enters a product as f16_rn(NF4[code] * absmax).
 * haff_nf4_quantize_f16: f16 W [N][K] (row stride ldw, 16-B aligned) -> packed / absmax, source row n written to row row_map[n]
 * (NULL: n) of both outputs. Codes: nearest NF4 value to w * (1/absmax) (a value on a midpoint takes the lower code; an all-zero
 * block has codes 7). double_quant 1: absmax goes through bitsandbytes' double quantisation (offset = mean absmax, summed in
 * double in a fixed order, stored to *offset (device f32); blocks of 256 of absmax - offset on the signed dynamic map);
 * 0: the raw absmax (*offset is still the mean). workspace: device, >= 4 * N * (K/64) bytes. */
int haff_nf4_quantize_f16(const void* W, long ldw, int N, int K, int double_quant, const int* row_map, void* packed, float* absmax,
                          float* offset, void* workspace, long workspace_bytes, void* stream);
/* f16 out row row_map[n] (NULL: n; row stride ldo, 16-B aligned) = f16_rn(NF4[code] * absmax) of stored row n */
int haff_nf4_dequant_f16(const void* packed, const float* absmax, int N, int K, const int* row_map, void* out, long ldo, void* stream);
/* The same values TRANSPOSED, for the dX products of NF4 fine-tuning: f16 out_t[k][row_map[n]] (NULL: n; K rows of stride ldo, 16-B
 * aligned, ldo % 8 == 0, ldo >= roundup(N, 8)) = f16_rn(NF4[code(n, k)] * absmax(n, k / 64)); columns N .. roundup(N, 8) - 1 are
 * zero-filled, columns from roundup(N, 8) on are not written. row_map: a permutation of 0 .. N - 1. packed 16-B aligned. K % 64,
 * ldo, misalignment: -1. */
int haff_nf4_dequant_t_f16(const void* packed, const float* absmax, int N, int K, const int* row_map, void* out_t, long ldo,
                           void* stream);
/* haff_gemm_f16 with NF4 weights for M <= 64 (decode steps, [SEG] rows, lm_head on the last rows): C = epi(A . dequant(W)^T), same
 * epilogue contract (bias, act, resid may alias C, row_map, out_f32, swiglu on [gate x16 | up x16] rows). Weight-streaming kernel,
 * fixed summation order (bitwise repeatable). M > 64: -2; K % 64, lda, misalignment, SwiGLU with N % 32 or resid: -1. */
int haff_gemm_nf4_f16(const void* A, long lda, const void* Wq, const float* absmax, void* C, long ldc, const float* bias,
                      const void* resid, long ldr, const int* row_map, int M, int N, int K, int act, int out_f32, int swiglu,
                      void* stream);
/* Unmerged LoRA adapters on an NF4 weight (serving adapters fitted on the NF4 base): y = x . deq(W)^T + scale * (x . A^T) . B^T.
 * A fused weight has nseg (1..4) row segments of seg_rows stored rows (seg_rows % 16 == 0): stored row n belongs to segment
 * (n / seg_rows) % nseg (q | k | v: 3 x H; [gate x16 | up x16]: 2 x 16; o / down: 1). A_cat f16 [8 nseg][lda >= K]: 8 rank rows per
 * segment (rank < 8 zero-padded, an unadapted segment's rows zero); B f16 [N][8]: each stored row's own coefficients, in the stored
 * row order. A_cat / B / t 16-B aligned, lda % 8 == 0. Layout violations: -1, before any launch.
 * haff_nf4_dequant_lora_f16: haff_nf4_dequant_f16 (same arguments, same refusals) with the update folded into the pass:
 *   out[row_map[n]][k] = f16_rn(fl32(d + fl32(scale * u))), d = fl32(NF4[code] * absmax), u = the fp32 sum over j = 0..7, in that
 *   order, of B[n][j] * A_cat[8 seg(n) + j][k] (each product exact, each add rounded once).
 * haff_gemm_nf4_lora_f16: haff_gemm_nf4_f16 (same arguments, same refusals) with scale * sum_j t[m][8 seg(n) + j] * B[n][j] added
 *   to the fp32 sums before bias, act, SwiGLU and resid; t = x . A_cat^T as f16 [M][ldt], ldt >= 8 nseg, ldt % 8 == 0. Bitwise
 *   repeatable. */
int haff_nf4_dequant_lora_f16(const void* packed, const float* absmax, int N, int K, const int* row_map, void* out, long ldo,
                              const void* A_cat, long lda, const void* B, int nseg, int seg_rows, float scale, void* stream);
int haff_gemm_nf4_lora_f16(const void* A, long lda, const void* Wq, const float* absmax, void* C, long ldc, const float* bias,
                           const void* resid, long ldr, const int* row_map, int M, int N, int K, int act, int out_f32, int swiglu,
                           const void* t, long ldt, const void* B, int nseg, int seg_rows, float scale, void* stream);
/* LLM.int8 language-model weights of the fp16 mode (load_in_8bit; csrc/gemm_int8.hip, arithmetic restated in quant.py). K % 64 == 0.
 * haff_int8_quantize_weight_f16: f16 W [N][K] (row stride ldw, 16-B aligned) -> CB int8 [.][K] = rint(w * (127 / SCB)) and
 * SCB f32 = max |W[n][:]| (0: all-zero codes), source row n written to row row_map[n] (NULL: n). CB 16-B aligned. */
int haff_int8_quantize_weight_f16(const void* W, long ldw, int N, int K, const int* row_map, void* CB, float* SCB, void* stream);
/* Row quantisation of f16 A [M][K] with outlier decomposition. Rows [s * seg_rows, (s + 1) * seg_rows) form segment s (a frame);
 * its first seg_valid[s] rows (NULL: all) OR their outlier columns (|a| >= threshold; threshold 0: none) into masks[s] (uint32
 * [S][K/32], bit c % 32 of word c / 32; never cleared here: zeroed by the caller for a fresh call, kept for sticky decode masks).
 * SCA[m] = max |a| over row m's non-outlier elements; CA[m] (int8, row stride ldca % 16 == 0) = rint(a * (127 / SCA[m])), 0 on
 * the columns of its segment's mask and on its own outliers (SCA 0: all zero); cols[s][0 .. ncols[s]) (int32 [S][K]) = the
 * segment's columns, ascending. masks may be NULL with threshold 0. */
int haff_int8_quantize_act_f16(const void* A, long lda, int M, int K, float threshold, int seg_rows, const int* seg_valid,
                               unsigned* masks, void* CA, long ldca, float* SCA, int* cols, int* ncols, void* stream);
/* The int8 product: Y = f16(f32(CA . CB^T) * 6.200012e-05f * SCA[m] * SCB[n] + bias[n]) (left to right, not contracted), then for a
 * row whose segment (m / seg_rows) has columns: Y = f16(Y + f16(sum over its columns c, ascending, in fp32, of A[m][c] *
 * f16(CB[n][c] * SCB[n] / 127))). Then haff_gemm_f16's epilogue on Y: act, resid (may alias C), row_map, out_f32, swiglu on
 * [gate x16 | up x16] rows. cols / ncols NULL: no outlier term (A may then be NULL). form 0: by M (<= 64 weight-streaming,
 * else tiled), 1: weight-streaming (M > 64: -2), 2: tiled. Every form gives the same bits for a row. */
int haff_gemm_int8_f16(const void* A, long lda, const void* CA, long ldca, const float* SCA, const void* CB, const float* SCB,
                       const int* cols, const int* ncols, int seg_rows, void* C, long ldc, const float* bias, const void* resid, long ldr,
                       const int* row_map, int M, int N, int K, int act, int out_f32, int swiglu, int form, void* stream);
/* Decode-sized product (M <= 16; with ssq_in: M <= 8, ssq_n <= 512, ssq_in 16-B aligned; K % 128 == 0) that carries Llama's RMSNorm between products without a norm kernel
 * (transformers LlamaDecoderLayer as reached from 2Haff/model/llava/model/language_model/llava_llama.py:93-102:
 * input_layernorm -> q/k/v_proj, post_attention_layernorm -> gate/up_proj). ssq_in != NULL: row m of A . W^T is scaled by
 * rsqrt(sum_{b < ssq_n} ssq_in[b][m] / K + eps) before the epilogue — W must have the norm weight folded into its columns
 * and A is the un-normalised residual stream. ssq_out != NULL (bf16 output, no SwiGLU): workgroup b writes
 * ssq_out[b][m] = sum over its output columns of bf16(C[m][n])^2 (m < 16), *n_parts_out (host int, may be NULL) = number of
 * workgroups — exactly what the next product's ssq_in / ssq_n take. Both arrays: DEVICE fp32 [parts][16]. */
int haff_gemm_bf16_rms(const void* A, long lda, const void* W, long ldw, void* C, long ldc, const float* bias,
                       const void* resid, long ldr, int M, int N, int K, int act, int out_f32, int swiglu,
                       const float* ssq_in, int ssq_n, float eps, float* ssq_out, int* n_parts_out, void* stream);
/* One KV-cached decode step of n_layers Llama layers at M <= 8 rows as ONE launch (csrc/decode_chain.hip): the five stages of
 * every transformers LlamaDecoderLayer (q|k|v product with input_layernorm carried in -> RoPE + cache append + attention ->
 * o_proj + residual -> gate|up SwiGLU with post_attention_layernorm carried in -> down_proj + residual; reached from
 * llava_llama.py:93-102 during LISA.py:443-450's greedy generate) are workgroup ranges of one grid chained by arrival counters:
 * a workgroup requests its weight slab before it waits for its inputs, so the weight stream does not drain at stage boundaries.
 * Replaces, per layer, haff_gemm_bf16_rms x4 + haff_decode_attention_rope_rows_bf16; same arithmetic statement for statement
 * (bit-identical where that path splits a head over 4 waves: 5..8 rows).
 *   layers: HOST array of n_layers haff_chain_layer {wqkv [3H][H] (input_layernorm gamma folded into the columns), wo [H][H],
 *           wgu [2F][H] (16-row [gate | up] groups, post_attention_layernorm gamma folded in), wd [H][F], kcache, vcache
 *           [M][tmax][H]} of DEVICE pointers, copied into the kernel arguments;
 *   x [M][H] bf16 residual stream, in place; stats0 f32 [M][2] {mean, rstd} of its rows on entry (haff_row_stats, rms);
 *   qkv [M][3H], att [M][H], g [M][F] bf16, ssq_a / ssq_b f32 [H/16][16] and ws f32 [H/16][2][16][16] (the partial tiles of
 *   o_proj / down_proj, whose K extent is split over two workgroups and added in a fixed order): scratch; cos_sin f32 [tmax][128];
 *   nk_rows device int32 [M] = position of the new token + 1;
 *   sync: DEVICE uint32 [haff_decode_chain_sync_words(n_layers, hidden)], zeroed ONCE by the caller — the launch re-zeroes its arrival
 *   counters (8 shards + 8 replicas per (layer, stage), a 128-byte line each), the last line holds a sticky flag set when a
 *   bounded wait ran out (the grid then drains with a garbage result): haff_decode_chain_status.
 * hidden % 256 == 0, ffn % 256 == 0, hidden == heads * 128, hidden <= 8192, M <= 8, n_layers <= 48, pointers 16-B aligned;
 * otherwise -2 / -1. per_stage_launches != 0: the same kernel as one launch per (layer, stage) — identical arithmetic without the
 * chaining (tests, A/B). Handed-off bytes travel as agent-scope (sc1) stores and loads, no fences. haff_decode_chain_supported: workgroups per layer of the launch, 0 = unsupported geometry.
 * haff_decode_chain_status (synchronises the stream): 0 = every wait so far was satisfied, 1 = one ran out. */
typedef struct haff_chain_layer { const void *wqkv, *wo, *wgu, *wd; void *kcache, *vcache; } haff_chain_layer;
int haff_decode_chain_bf16(const haff_chain_layer* layers, int n_layers, int M, int hidden, int ffn, int heads, void* x,
                           void* qkv, void* att, void* g, float* ssq_a, float* ssq_b, float* ws, const float* stats0, float eps,
                           const float* cos_sin, const int* nk_rows, int tmax, float scale, unsigned* sync,
                           int per_stage_launches, void* stream);
int haff_decode_chain_supported(int M, int hidden, int ffn, int heads, int n_layers);
int haff_decode_chain_sync_words(int n_layers, int hidden);
int haff_decode_chain_status(const unsigned* sync, int n_layers, void* stream);
/* haff_gemm_bf16 with a gather on the A side: logical row m reads A row a_map[m] (0 <= a_map[m] < a_rows). Runs the
 * window-unpartition projection over real tokens only (image_encoder.py:186-188,291-318 drop the padded rows right
 * after proj). */
int haff_gemm_bf16_gather(const void* A, long lda, const int* a_map, long a_rows, const void* W, long ldw, void* C,
                          long ldc, const float* bias, const void* resid, long ldr, const int* row_map, int M, int N,
                          int K, int act, int out_f32, int swiglu, void* stream);
/* haff_gemm_bf16 with a LayerNorm / RMSNorm folded into the product: the normalised activations never exist in HBM.
 *   C[m][n] = act( rstd_m * (sum_k A[m][k] W'[n][k] - mean_m * colsum[n]) + bias'[n] )
 * with W' = W * gamma (column scaling, done once by the caller), bias' = bias + W.beta, colsum[n] = sum_k W'[n][k]
 * (null for RMSNorm), ln_stats[m] = {mean_m, rstd_m} from haff_row_stats. Replaces norm1 -> qkv and norm2 -> lin1 of the
 * SAM blocks (image_encoder.py:179,191), the RMSNorms in front of Llama's qkv / gate-up, CLIP's layer_norm1/2. */
int haff_gemm_bf16_ln(const void* A, long lda, const void* W, long ldw, void* C, long ldc, const float* bias,
                      const void* resid, long ldr, const int* row_map, const float* ln_stats, const float* ln_colsum,
                      int M, int N, int K, int act, int out_f32, int swiglu, void* stream);
/* Product (optionally with a folded norm: ln_stats / ln_colsum as above, or both null) whose bf16 output is scattered HEAD-MAJOR:
 * the windowed q|k|v projection of a ViT-H block (image_encoder.py:223-224 the qkv Linear, :263-288 window_partition, :238-239 the
 * reshape into heads) writes q, k, v of every (window, head) as ONE contiguous [tokens][d] block, so the window attention's K / V
 * staging reads whole 128-B lines. Product column n = part * (heads * d) + h * d + c of product row m is stored at
 *   C[part * part_stride + h * head_stride + row_map[m] * d + c]      (bf16 elements; row_map[m] < 0 drops the row)
 * i.e. with row_map[m] = window * heads * n_tok + token, head_stride = n_tok * d, part_stride = (windows + 1) * heads * n_tok * d,
 * C is [part][window][head][token][d] with one spare window whose token 0 holds the pad token (the caller writes it).
 * Whole 256 x 256 tiles only (M % 256 == 0, N % 256 == 0, K % 64 == 0), N == parts * heads * d with parts <= 3, d % 8 == 0;
 * otherwise HAFF_ERR_UNSUPPORTED (-2): the caller keeps the token-major layout (haff_gemm_bf16_ln / haff_gemm_bf16 with a row map). */
int haff_gemm_bf16_heads(const void* A, long lda, const void* W, long ldw, void* C, const float* bias, const int* row_map,
                         const float* ln_stats, const float* ln_colsum, int M, int N, int K, int d, int heads, long part_stride,
                         long head_stride, void* stream);
/* How many workgroups the persistent 8-wave tile launches enqueued ON `stream` take from now on (256 = one per CU, the default;
 * read when a launch is enqueued or captured). Scheduling, not arithmetic: results are bit-identical for every value. The caller
 * lowers it for the launches of ONE stream so that kernels of another stream find free CUs while they run — LisaMI355.evaluate does
 * for the later passes of the SAM encoder (image_encoder.py:107-121) on its encoder stream, which run beside the HBM-bound decode
 * steps (LISA.py:443-450) of the caller's stream. The setting is per stream (round 5's was process-wide: two models or two host
 * threads raced on it): launches on other streams are unaffected. cap: a multiple of 8 in 8..256 (a workgroup's tiles stay on one
 * XCD); any other value changes nothing (a query). Returns the stream's previous cap (256 when it had none), or
 * HAFF_ERR_UNSUPPORTED (-2) when 32 streams are capped at once. Setting 256 releases the stream's entry. */
int haff_gemm_stream_cap(void* stream, int cap);
/* Llama prefill q|k|v projection with rotate-half RoPE and the KV-cache append in the epilogue (transformers
 * LlamaAttention.forward via llava_llama.py:93-102) — replaces haff_gemm_bf16 + haff_rope_cache on prefill-sized batches.
 * A bf16 [B*T][K]; Wp bf16 [3*H*d][K]: the fused q|k|v weights with the rows of every 256-row tile permuted — natural tile row
 * wn*64 + t*16 + i holds logical row (wn>>1)*128 + (t>>1)*64 + (wn&1)*32 + (t&1)*16 + i (wn, t in 0..3, i in 0..15), so that a
 * lane owns a column and its rotate-half partner; q_out bf16 [B*T][ldq] receives the rotated q (H*d columns); kcache / vcache
 * bf16 [B][Tmax][H*d] receive the rotated k and v at rows pos0 .. pos0+T-1; cos_sin f32 [Tmax][d] = cos | sin.
 * d == 128, (H*d) % 256 == 0, K % 64 == 0; otherwise HAFF_ERR_UNSUPPORTED (-2). */
int haff_gemm_bf16_qkv_rope(const void* A, long lda, const void* Wp, long ldw, void* q_out, long ldq, void* kcache,
                            void* vcache, const float* cos_sin, int B, int T, int Tmax, int pos0, int H, int d, int K,
                            void* stream);
/* residual product that also emits the LayerNorm statistics of its output rows (proj / lin2 of a SAM block,
 * image_encoder.py:186-193): C = A.W^T + bias + resid (bf16; C may alias resid; a_map: optional A-side gather as in
 * haff_gemm_bf16_gather); stat_out f32 [M][N/64][2] = {sum, sum of squares} of each 64-column slice of the fp32 results.
 * haff_row_stats_finalize turns them into the {mean, rstd} rows haff_gemm_bf16_ln takes. Whole 256 x 256 tiles only
 * (M % 256 == 0, N % 256 == 0, K % 64 == 0), else HAFF_ERR_UNSUPPORTED (-2): the caller keeps haff_row_stats. */
int haff_gemm_bf16_rowstats(const void* A, long lda, const int* a_map, long a_rows, const void* W, long ldw, void* C,
                            long ldc, const float* bias, const void* resid, long ldr, int M, int N, int K,
                            float* stat_out, void* stream);
/* haff_gemm_bf16_rowstats on an FP32 residual stream (the timed mode's option `fp32_stream`): X32 f32
 * [M][ldx] is read and X32 + A.W^T + bias written back IN PLACE in fp32 (the residual adds of image_encoder.py:186-193 no longer
 * round the stream to bf16 twice per block); C16 bf16 [M][ldc] receives the same sums rounded once — the MFMA operand of the next
 * haff_gemm_bf16_ln, whose folded LayerNorm takes stat_out (f32 [M][N/64][2], from the fp32 sums) through
 * haff_row_stats_finalize. a_map: optional A-side gather. Whole 256 x 256 tiles only (M % 256 == 0, N % 256 == 0, K % 64 == 0),
 * ldx % 4 == 0, bias required; otherwise HAFF_ERR_UNSUPPORTED (-2) / HAFF_ERR_BAD_ARG (-1). */
int haff_gemm_bf16_rowstats32(const void* A, long lda, const int* a_map, long a_rows, const void* W, long ldw, float* X32,
                              long ldx, void* C16, long ldc, const float* bias, int M, int N, int K, float* stat_out,
                              void* stream);
/* parity-mode twin: everything f32. K % 4 == 0, lda/ldw % 4 == 0. */
int haff_gemm_f32(const float* A, long lda, const float* W, long ldw, float* C, long ldc, const float* bias,
                  const float* resid, long ldr, const int* row_map, int M, int N, int K, int act, int swiglu,
                  void* stream);

/* ---- fused attention: out = softmax(scale * q.k^T + bias [+ causal mask]) . v ---------------------------------
 * Replaces SAM Attention.forward + add_decomposed_rel_pos (image_encoder.py:235-260,354-392), CLIPAttention,
 * LlamaAttention (prefill and KV-cached decode) and the SAM decoder Attention (transformer.py:220-242).
 * q/k/v/o: [B][H][N][d] views given by (batch, head, token) strides, unit stride on d; d % 8 == 0 (bf16: d <= 128).
 * causal != 0: key j visible to query i iff j <= i + q_pos0.
 * relh/relw (null = no bias): f32 [B*H][Nq][S] from haff_relpos_tables; key j -> (kh, kw) = (j / S, j % S).
 * bf16 kernel supports S == 64 (one KV tile per key-grid row) or S <= 32. */
int haff_attention_bf16(const void* q, long q_sb, long q_sh, long q_st, const void* k, long k_sb, long k_sh, long k_st,
                        const void* v, long v_sb, long v_sh, long v_st, void* o, long o_sb, long o_sh, long o_st,
                        int B, int H, int Nq, int Nk, int d, float scale, int causal, int q_pos0,
                        const float* relh, const float* relw, int S, void* stream);
/* fp16 instance of haff_attention_bf16 (q/k/v/o f16; the probabilities enter the P.V product as f16) */
int haff_attention_f16(const void* q, long q_sb, long q_sh, long q_st, const void* k, long k_sb, long k_sh, long k_st,
                       const void* v, long v_sb, long v_sh, long v_st, void* o, long o_sb, long o_sh, long o_st,
                       int B, int H, int Nq, int Nk, int d, float scale, int causal, int q_pos0,
                       const float* relh, const float* relw, int S, void* stream);
int haff_attention_f32(const float* q, long q_sb, long q_sh, long q_st, const float* k, long k_sb, long k_sh, long k_st,
                       const float* v, long v_sb, long v_sh, long v_st, float* o, long o_sb, long o_sh, long o_st,
                       int B, int H, int Nq, int Nk, int d, float scale, int causal, int q_pos0,
                       const float* relh, const float* relw, int S, void* stream);

/* KV-cached decode over RAGGED caches (batched prompts of different lengths; reference padding rules:
 * 2Haff/utils/dataset.py:90-93,144-150): one query per (batch, head); batch b attends its first nk_rows[b] cached keys
 * (DEVICE int32 [B], 1 <= nk_rows[b] <= Nk). q/o: [B][H][d] with (batch, head) strides; k/v as haff_attention_bf16. */
int haff_attention_decode_rows_bf16(const void* q, long q_sb, long q_sh, const void* k, long k_sb, long k_sh, long k_st,
                                    const void* v, long v_sb, long v_sh, long v_st, void* o, long o_sb, long o_sh, int B,
                                    int H, int Nk, int d, float scale, const int* nk_rows, void* stream);
int haff_attention_decode_rows_f16(const void* q, long q_sb, long q_sh, const void* k, long k_sb, long k_sh, long k_st,
                                   const void* v, long v_sb, long v_sh, long v_st, void* o, long o_sb, long o_sh, int B,
                                   int H, int Nk, int d, float scale, const int* nk_rows, void* stream);
int haff_attention_decode_rows_f32(const float* q, long q_sb, long q_sh, const float* k, long k_sb, long k_sh, long k_st,
                                   const float* v, long v_sb, long v_sh, long v_st, float* o, long o_sb, long o_sh, int B,
                                   int H, int Nk, int d, float scale, const int* nk_rows, void* stream);
/* the same decode position with RoPE and the KV-cache append fused in: replaces haff_rope_cache_rows +
 * haff_attention_decode_rows_bf16 (transformers LlamaAttention with a KV cache, llava_llama.py:93-102). qkv [B][ld]: raw
 * q | k | v of the new position (H x d each); caches [B][Tmax][H*d]; cos_sin f32 [Tmax][d]; nk_rows[b] = new position + 1
 * (DEVICE int32 [B]); out [B][H*d]; d == 128. Results are bit-identical to the two-kernel path. */
int haff_decode_attention_rope_rows_bf16(const void* qkv, long ld, void* kcache, void* vcache, const float* cos_sin, void* out,
                                         int B, int H, int d, int Tmax, float scale, const int* nk_rows, void* stream);
int haff_decode_attention_rope_rows_f16(const void* qkv, long ld, void* kcache, void* vcache, const float* cos_sin, void* out,
                                        int B, int H, int d, int Tmax, float scale, const int* nk_rows, void* stream);
/* decomposed rel-pos terms (image_encoder.py:376-384, from the UNSCALED q, :244-248):
 * relh[bh][q][kh] = q . Rh[qh - kh + S - 1], relw[bh][q][kw] = q . Rw[qw - kw + S - 1]; N = S*S queries.
 * tab_*: [2S-1][d] (f32 for the generic entry, bf16 for the MFMA entry). */
int haff_relpos_tables(const void* q, long q_sb, long q_sh, long q_st, const float* tab_h, const float* tab_w,
                       float* relh, float* relw, int B, int H, int S, int d, int dtype, void* stream);
int haff_relpos_tables_bf16(const void* q, long q_sb, long q_sh, long q_st, const void* tab_h, const void* tab_w,
                            float* relh, float* relw, int B, int H, int S, int d, void* stream);

/* flash attention pair of the fine-tune path (transformers LlamaAttention under autograd; row a16, LISA.py:175-430):
 * haff_attention_lse_bf16 = haff_attention_bf16 (no bias) that also returns lse f32 [B][H][Nq] = log2 sum_k 2^(scale*log2(e)*q.k)
 * over the visible keys; haff_attention_bwd_bf16 = dq, dk, dv from q, k, v, o, dout and lse without the probabilities ever
 * existing in HBM (d == 128; bitwise repeatable: no atomics). q / o / dout / dq: [B][Nq][ld], k / v / dk / dv: [B][Nk][ld],
 * head h at columns h*128 (ld >= H*128, ld % 8 == 0, 16-byte aligned bases); workspace f32, 16-byte aligned, with at least
 * roundup(B*H*Nq, 4) + B*H*128*roundup(Nq, 64) values (B*H*(Nq + 3 + 128*roundup(Nq, 64)) is always enough). Refused with
 * HAFF_ERR_BAD_ARG before any launch, by all four entry points: a null or misaligned operand, result, lse or workspace; causal with
 * q_pos0 < 0 (a query that sees no key has no log-sum-exp, and the backward's key block 0 must be seen by every query block). */
int haff_attention_lse_bf16(const void* q, long q_sb, long q_sh, long q_st, const void* k, long k_sb, long k_sh, long k_st,
                            const void* v, long v_sb, long v_sh, long v_st, void* o, long o_sb, long o_sh, long o_st, int B, int H,
                            int Nq, int Nk, int d, float scale, int causal, int q_pos0, float* lse, void* stream);
int haff_attention_bwd_bf16(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                            void* dq, void* dk, void* dv, float* workspace, long workspace_elems, long ld, int B, int H, int Nq,
                            int Nk, int d, float scale, int causal, int q_pos0, void* stream);
/* fp16 fine-tuning: the same pair on IEEE binary16 operands (f16 MFMA, fp32 accumulation and statistics) */
int haff_attention_lse_f16(const void* q, long q_sb, long q_sh, long q_st, const void* k, long k_sb, long k_sh, long k_st,
                           const void* v, long v_sb, long v_sh, long v_st, void* o, long o_sb, long o_sh, long o_st, int B, int H,
                           int Nq, int Nk, int d, float scale, int causal, int q_pos0, float* lse, void* stream);
int haff_attention_bwd_f16(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse,
                           void* dq, void* dk, void* dv, float* workspace, long workspace_elems, long ld, int B, int H, int Nq,
                           int Nk, int d, float scale, int causal, int q_pos0, void* stream);

/* TN product of the fine-tune step: out [N1][N2] = A^T . B, A [M][lda] (N1 columns), B [M][ldb] (N2 columns), bf16, contraction
 * over the M rows — the weight gradient dW = dY^T . X of a trainable Linear (torch.nn.Linear under autograd: text_hidden_fcs and
 * the mask decoders, train_ds.py:232-244) without transposed copies of dY and X (csrc/gemm_tn.hip: fragments through the
 * transposing LDS read). N1, N2, lda, ldb % 8 == 0, 16-byte aligned bases, else HAFF_ERR_UNSUPPORTED (the caller then takes
 * haff_transpose + haff_gemm_bf16). out contiguous, bf16 or f32; workspace f32, 16-byte aligned, with at least
 * haff_gemm_tn_workspace_elems(M, N1, N2) values (split partials, added in index order: repeatable to the bit); a null,
 * misaligned or shorter workspace is HAFF_ERR_BAD_ARG. haff_gemm_tn_workspace_elems answers HAFF_ERR_BAD_ARG for a size <= 0
 * and HAFF_ERR_UNSUPPORTED for a count past INT_MAX. */
int haff_gemm_tn_workspace_elems(long M, int N1, int N2);
int haff_gemm_tn_bf16(const void* A, long lda, const void* B, long ldb, long M, int N1, int N2, float* workspace,
                      long workspace_elems, void* out, int out_f32, void* stream);
/* fp16 fine-tuning: A, B and a 16-bit out IEEE binary16 */
int haff_gemm_tn_f16(const void* A, long lda, const void* B, long ldb, long M, int N1, int N2, float* workspace,
                     long workspace_elems, void* out, int out_f32, void* stream);

/* rank-r adapter path of the fine-tune step (peft LoRA on q_proj / v_proj: 2Haff/train_ds.py:192-230; RoPE of the adapted
 * projections: llava_llama.py -> transformers LlamaAttention). bf16, head dim d == 128, rank <= 8 per adapter; see csrc/lora.hip.
 * tT / dtT: [16][ld] = the TRANSPOSED rank activations, rows 0..7 the q adapter, 8..15 the v adapter (unused ranks zero);
 * Bq / Bv: [H][8] (ldb == 8, unused rank columns zero); A2: [16][K] = [Aq; 0; Av; 0]; cos_sin f32 [T][128], position = row % T.
 * haff_lora_qkv_rope_fwd: q_out = rope(qkv[:, :H] + scale * t_q.Bq^T), k_out = rope(qkv[:, H:2H]), v_out = qkv[:, 2H:] + scale * t_v.Bv^T
 * haff_lora_qkv_rope_bwd: dqkv [M][3H] = [rope^T dq | rope^T dk | dv] (the adjoint of the q|k|v product's output)
 * haff_lora_dx:           dx (+)= scale * keep .* (dt . A2)   (keep: optional dropout mask values [M][K])
 * haff_lora_tn:           out = scale * sT . big  (sT [R][lds] with R = 8 or 16, lds % 8 == 0, lds >= roundup(M, 16), padding finite; big [M][N]; contraction over the M
 *                         rows; out [j_valid][N] or, transposed, [N][j_valid], bf16 or f32) — the dA / dB contraction without a
 *                         transposed copy of either operand; workspace f32 with haff_lora_tn_workspace_elems values;
 *                         row-block partials are added in index order (deterministic). */
int haff_lora_qkv_rope_fwd(const void* qkv, long ld_qkv, const void* tT, long ldt, const void* Bq, const void* Bv, int ldb,
                           const float* cos_sin, void* q_out, void* k_out, void* v_out, long ldo, long M, int H, int d, int T,
                           float scale, void* stream);
int haff_lora_qkv_rope_bwd(const void* dq, const void* dk, const void* dv, long ld_in, const float* cos_sin, void* dqkv,
                           long ld_out, long M, int H, int d, int T, void* stream);
int haff_lora_dx(const void* dtT, long ldt, const void* A2, long lda, const void* keep, long ldk, void* dx, long ldx,
                 int accumulate, long M, int K, float scale, void* stream);
/* the same with TWO dropout masks — peft gives each adapted Linear its own lora_dropout (train_ds.py:218-230):
 * dx (+)= scale * (keep_q o (dt[0:8]^T . A2[0:8]) + keep_v o (dt[8:16]^T . A2[8:16])). */
int haff_lora_dx2(const void* dtT, long ldt, const void* A2, long lda, const void* keep_q, const void* keep_v, long ldk, void* dx,
                  long ldx, int accumulate, long M, int K, float scale, void* stream);
int haff_lora_tn_workspace_elems(long M, int R, int N);
int haff_lora_tn(const void* sT, long lds, int R, const void* big, long ldb, long M, int N, float* workspace,
                 long workspace_elems, void* out, long ldo, int out_f32, int transposed, int j_valid, float scale, void* stream);
/* fp16 fine-tuning: the same five entry points on IEEE binary16 operands, masks and results (haff_lora_tn_workspace_elems serves both) */
int haff_lora_qkv_rope_fwd_f16(const void* qkv, long ld_qkv, const void* tT, long ldt, const void* Bq, const void* Bv, int ldb,
                               const float* cos_sin, void* q_out, void* k_out, void* v_out, long ldo, long M, int H, int d, int T,
                               float scale, void* stream);
int haff_lora_qkv_rope_bwd_f16(const void* dq, const void* dk, const void* dv, long ld_in, const float* cos_sin, void* dqkv,
                               long ld_out, long M, int H, int d, int T, void* stream);
int haff_lora_dx_f16(const void* dtT, long ldt, const void* A2, long lda, const void* keep, long ldk, void* dx, long ldx,
                     int accumulate, long M, int K, float scale, void* stream);
int haff_lora_dx2_f16(const void* dtT, long ldt, const void* A2, long lda, const void* keep_q, const void* keep_v, long ldk, void* dx,
                      long ldx, int accumulate, long M, int K, float scale, void* stream);
int haff_lora_tn_f16(const void* sT, long lds, int R, const void* big, long ldb, long M, int N, float* workspace,
                     long workspace_elems, void* out, long ldo, int out_f32, int transposed, int j_valid, float scale, void* stream);
/* LoRA on every Llama projection (--lora_target_modules). Rank <= 8 per adapter, B operands [rows][8] (unused rank columns zero).
 * haff_lora_qkv3_rope_fwd: haff_lora_qkv_rope_fwd with a k adapter: tT [24][ldt], rows 16..23 the k adapter's ranks;
 *                          k_out = rope(qkv[:, H:2H] + scale * t_k.Bk^T).
 * haff_lora_dx3:           dx (+)= scale * sum over the three adapters of keep_a o (dt_a . A_a), dtT / A3 [24][.] in the same
 *                          order (q, v, k); masks: none, keep_q alone (one mask for all three), or all three.
 * haff_lora_out:           y [M][N] += scale * t.B^T, tT [8][ldt] (ldt % 4 == 0, ldt >= roundup(M, 4), padding finite), B [N][8]:
 *                          an adapted Linear's update on the frozen product's output (o_proj / down_proj, residual included).
 * haff_lora_gu_swiglu:     gu [M][2F] (interleaved [gate x16 | up x16]) += scale * update IN PLACE, the gate columns from
 *                          t^T rows 0..7 and Bg [F][8], the up columns from rows 8..15 and Bu [F][8]; y [M][F] = silu(g') * u'
 *                          of the stored (rounded) g', u'. */
int haff_lora_qkv3_rope_fwd(const void* qkv, long ld_qkv, const void* tT, long ldt, const void* Bq, const void* Bv, const void* Bk,
                            int ldb, const float* cos_sin, void* q_out, void* k_out, void* v_out, long ldo, long M, int H, int d,
                            int T, float scale, void* stream);
int haff_lora_dx3(const void* dtT, long ldt, const void* A3, long lda, const void* keep_q, const void* keep_v, const void* keep_k,
                  long ldk, void* dx, long ldx, int accumulate, long M, int K, float scale, void* stream);
int haff_lora_out(const void* tT, long ldt, const void* B, void* y, long ldy, long M, int N, float scale, void* stream);
int haff_lora_gu_swiglu(const void* tT, long ldt, const void* Bg, const void* Bu, void* gu, long ldg, void* y, long ldy, long M,
                        int F, float scale, void* stream);
int haff_lora_qkv3_rope_fwd_f16(const void* qkv, long ld_qkv, const void* tT, long ldt, const void* Bq, const void* Bv,
                                const void* Bk, int ldb, const float* cos_sin, void* q_out, void* k_out, void* v_out, long ldo,
                                long M, int H, int d, int T, float scale, void* stream);
int haff_lora_dx3_f16(const void* dtT, long ldt, const void* A3, long lda, const void* keep_q, const void* keep_v,
                      const void* keep_k, long ldk, void* dx, long ldx, int accumulate, long M, int K, float scale, void* stream);
int haff_lora_out_f16(const void* tT, long ldt, const void* B, void* y, long ldy, long M, int N, float scale, void* stream);
int haff_lora_gu_swiglu_f16(const void* tT, long ldt, const void* Bg, const void* Bu, void* gu, long ldg, void* y, long ldy,
                            long M, int F, float scale, void* stream);

/* fused SAM WINDOW attention with the decomposed rel-pos bias computed in the kernel (one pass over HBM; replaces
 * haff_relpos_tables_bf16 + haff_attention_bf16 for the 28 windowed ViT-H blocks): Attention.forward
 * (image_encoder.py:235-260) + add_decomposed_rel_pos (:354-392) + get_rel_pos with q_size == k_size (:322-351).
 * q/k/v/o: bf16 [n_windows][H][S*S][d] views given by (window, head, token) strides; tab_*: bf16 [2S-1][d].
 * grid_h/grid_w > 0: windows tile images of grid_h x grid_w tokens; window tokens beyond the grid are pads that the
 * caller never wrote — their q/k/v are read from token row pad_token (= projection of a zero token = the qkv bias;
 * window_partition pads AFTER norm1, image_encoder.py:179-183,263-288). grid_h == 0: every token is real.
 * Supported geometry: S == 14, d == 80; otherwise HAFF_ERR_UNSUPPORTED (-2) and the caller takes the generic pair. */
int haff_window_attention_bf16(const void* q, long q_sb, long q_sh, long q_st, const void* k, long k_sb, long k_sh,
                               long k_st, const void* v, long v_sb, long v_sh, long v_st, void* o, long o_sb,
                               long o_sh, long o_st, int n_windows, int H, int S, int d, float scale,
                               const void* tab_h, const void* tab_w, int grid_h, int grid_w, long pad_token,
                               void* stream);
/* fp16 instance: q / k / v / o and tab_h / tab_w f16 */
int haff_window_attention_f16(const void* q, long q_sb, long q_sh, long q_st, const void* k, long k_sb, long k_sh,
                              long k_st, const void* v, long v_sb, long v_sh, long v_st, void* o, long o_sb,
                              long o_sh, long o_st, int n_windows, int H, int S, int d, float scale,
                              const void* tab_h, const void* tab_w, int grid_h, int grid_w, long pad_token,
                              void* stream);

/* fused SAM GLOBAL attention (the 4 global ViT-H blocks, 64 x 64 tokens): Attention.forward (image_encoder.py:235-260) +
 * add_decomposed_rel_pos (:354-392), the rel-pos terms computed in the kernel's prologue from the parameter tables (replaces
 * haff_relpos_tables_bf16 + haff_attention_bf16: no fp32 [B*H][N][S] tables cross HBM). q/k/v/o: bf16 [B][H][S*S][d] views by
 * (batch, head, token) strides; k and v must share one row layout (same strides, v at a non-negative offset behind k — the
 * fused qkv projection output); tab_*: bf16 [2S-1][d]. Supported geometry: S == 64, d == 80; otherwise
 * HAFF_ERR_UNSUPPORTED (-2) and the caller takes the two-kernel path. */
int haff_global_attention_bf16(const void* q, long q_sb, long q_sh, long q_st, const void* k, long k_sb, long k_sh,
                               long k_st, const void* v, long v_sb, long v_sh, long v_st, void* o, long o_sb,
                               long o_sh, long o_st, int B, int H, int S, int d, float scale,
                               const void* tab_h, const void* tab_w, void* stream);
/* fp16 instance: q / k / v / o and tab_h / tab_w f16 */
int haff_global_attention_f16(const void* q, long q_sb, long q_sh, long q_st, const void* k, long k_sb, long k_sh,
                              long k_st, const void* v, long v_sb, long v_sh, long v_st, void* o, long o_sb,
                              long o_sh, long o_st, int B, int H, int S, int d, float scale,
                              const void* tab_h, const void* tab_w, void* stream);

/* ---- row norms ----------------------------------------------------------------------------------------------
 * haff_layernorm: nn.LayerNorm / LayerNorm2d on channels-last rows (common.py:31-43; image_encoder.py:179,191;
 * transformer.py:134-144; CLIP layer norms). in_map (int32[rows], may be null): out row i normalises in row
 * in_map[i]; negative = zero row (window_partition's zero pad AFTER norm1, image_encoder.py:179-183,276-288).
 * haff_rmsnorm: LlamaRMSNorm (fp32 variance). w, b: f32[C]. C % 8 == 0, C <= 8192 (wider: HAFF_ERR_UNSUPPORTED), ldx / ldy % 8 == 0.
 * dtype: 0 = bf16 rows, 1 = f32 rows, 2 = f32 x -> bf16 y (an fp32 residual stream feeding a bf16 product), 3 = f16 rows.
 * Columns C .. ld of x are not read and those of y not written, nor any row past `rows`. in_map is a DEVICE array: the caller
 * guarantees that every non-negative entry is a row of x; nothing checks it. */
int haff_layernorm(const void* x, long ldx, void* y, long ldy, const float* w, const float* b, const int* in_map,
                   int rows, int C, float eps, int dtype, void* stream);
int haff_rmsnorm(const void* x, long ldx, void* y, long ldy, const float* w, int rows, int C, float eps, int dtype,
                 void* stream);
/* per-row {mean, rstd} only (rms != 0: {0, rsqrt(mean(x^2)+eps)}): stats f32 [rows][2]; dtype 0 = bf16, 1 = f32, 3 = f16, any
 * other code (2 included: there is no output row to round) returns HAFF_ERR_BAD_ARG. Same C / ldx rules as the norms. */
int haff_row_stats(const void* x, long ldx, float* stats, int rows, int C, float eps, int rms, int dtype, void* stream);

/* stats[rows][2] = {mean, rstd} from haff_gemm_bf16_rowstats' partials f32 [rows][slots][2] (slots added in order); C = row length.
 * Sums, the division by C and E[x^2] - mean^2 (clamped at 0) are in double; only the two results are rounded to fp32. */
int haff_row_stats_finalize(const float* partials, float* stats, int rows, int slots, int C, float eps, void* stream);

/* ---- data movement ------------------------------------------------------------------------------------------ */
/* conv(k=s=P) rows: x [B][Cin][Hin][Win] -> out [B*gh*gw][Kp], column (c*P+ky)*P+kx, zero beyond Cin*P*P.
 * SAM PatchEmbed.proj (image_encoder.py:418-426), CLIP patch_embedding. */
int haff_patchify_nchw(const void* x, void* out, int B, int Cin, int Hin, int Win, int P, int gh, int gw, int Kp,
                       int in_dtype, int out_dtype, void* stream);
/* same rows straight from uint8 NHWC frames [B][Hf][Wf][3]: (x-mean)/std, zero pad right/bottom
 * (inference.preprocess, inference.py:91-105). mean3/std3: HOST pointers to 3 floats (0..255 scale). */
int haff_patchify_u8(const void* frames, void* out, int B, int Hf, int Wf, int P, int gh, int gw, int Kp,
                     const float* mean3, const float* std3, int out_dtype, void* stream);
/* neck 3x3 conv pad 1 (image_encoder.py:100-106): x [B][H][W][C] -> [B*H*W][9*C], column (ky*3+kx)*C+c */
int haff_im2col3x3(const void* x, void* out, int B, int H, int W, int C, int dtype, void* stream);
/* embed_tokens gather + image-feature splice (llava_arch.py:185-208,252-256): ids int64 [B][L] with the sentinel
 * at img_pos[b]; out [B][L+n_img-1][Hd] */
int haff_embed_splice(const long* ids, const int* img_pos, const void* embed, const void* img, void* out, int B, int L,
                      int n_img, int Hd, int dtype, void* stream);
/* rotate-half RoPE on q,k in place (qkv [B*Tq][ld]: q | k | v) + KV-cache append at positions pos0..pos0+Tq-1
 * (caches [B][Tmax][Hkv*d]); cos_sin f32 [Tmax][d] = cos(d/2) | sin(d/2). d % 16 == 0. */
int haff_rope_cache(void* qkv, long ld, void* kcache, void* vcache, const float* cos_sin, int B, int Tq, int Hq, int Hkv,
                    int d, int pos0, int Tmax, int dtype, void* stream);
/* Shared-prefix K/V broadcast (LisaMI355.evaluate(offset=): several prompt rows on one frame): positions 0 .. P-1 of k_src / v_src
 * [F][tmax_src][H], row frame_of[b], are copied into row b of k_dst / v_dst [B][tmax_dst][H]; both tensors in one launch, nothing
 * is written at positions >= P. Row strides in ELEMENTS (>= P*H, a whole number of 16-byte units); unit stride on H and H elements
 * between positions in both caches; H * elem % 16 == 0; the four pointers 16-byte aligned; P >= 1 (P <= tmax of both caches is the
 * caller's contract); dtype 0 bf16 / 1 f32 / 3 f16. frame_of: DEVICE int32 [B], validated by the caller against F; an entry outside
 * [0, F) is never dereferenced (that row is left as it was). 16-byte loads and stores only; bound: the 2*B*P*H*elem bytes written. */
int haff_kv_prefix_broadcast(const void* k_src, const void* v_src, long src_row_stride, void* k_dst, void* v_dst,
                             long dst_row_stride, const int* frame_of, int B, int F, int P, int H, int dtype, void* stream);
/* same with a per-row start position: row b's Tq new positions begin at pos0_rows[b] (DEVICE int32 [B];
 * pos0_rows[b] + Tq <= Tmax is the caller's contract) — greedy decode of right-padded prompts of different lengths */
int haff_rope_cache_rows(void* qkv, long ld, void* kcache, void* vcache, const float* cos_sin, int B, int Tq, int Hq,
                         int Hkv, int d, const int* pos0_rows, int Tmax, int dtype, void* stream);
/* greedy token: first index of the row maximum (generate(num_beams=1), LISA.py:443-450), in torch.argmax's order: a NaN
 * is greater than every number, so a row that holds NaNs gives the index of its first NaN. out[r] is always in [0, V). */
int haff_argmax_rows(const float* x, long ld, long* out, int rows, int V, void* stream);
/* One generated token per row of the greedy decode loop, on the device (replaces the per-step host bookkeeping of
 * transformers' generate as used by LISA.py:443-450; sits inside the decode hipGraph). Row b, step s = steps[b]:
 * token = *use_forced ? forced[b][s] : nxt_raw[b]; pad if finished[b]; out_ids[b][lens[b]+s] = token; finished[b] |= token == eos;
 * tok[b] = token; pos[b] = t_rows[b]+s; nk[b] = pos[b]+1; for s >= 1 and h1 != NULL: hidden[b][t_rows[b]+s-1] = h1[b]
 * (row_bytes bytes, multiple of 16); steps[b] = s+1. All pointers device memory; hid_sb = bytes between rows b of hidden. */
int haff_decode_book(const long* nxt_raw, const long* forced, long forced_ld, const int* use_forced, int* steps,
                     unsigned char* finished, long* out_ids, long out_ld, const long* lens, const int* t_rows, long* tok,
                     int* pos, int* nk, const void* h1, void* hidden, long hid_sb, long row_bytes, long pad, long eos, int B,
                     void* stream);
/* out[r] = a[r] + b[r % mod]  (PE adds, transformer.py:166-178; src + dense prompt, mask_decoder.py:141) */
int haff_add_bcast(const void* a, const void* b, void* out, long rows, int C, int mod, int dtype, void* stream);
/* row softmax to f32 (taxonomy head, mask_decoder.py:177) */
int haff_softmax_rows(const void* x, float* out, int rows, int C, int dtype, void* stream);

/* ---- SAM decoder tail + post-processing ------------------------------------------------------------------------
 * haff_upscale_mask: LayerNorm2d(64) -> GELU -> ConvTranspose2d(64->32,k2,s2) -> GELU -> dot with the hypernetwork
 * vector of mask token 0 (mask_decoder.py:58-64,153-165,110-114). up1 [n*h*w][4*64] = output of the first
 * transposed conv as GEMM, columns (dy*2+dx)*64+co; w2 f32 [64][4*32] column (dy2*2+dx2)*32+c2; hyper f32 [n][32];
 * out f32 [n][4h][4w]. dtype (of up1): 0 bf16, 1 f32, 3 f16. */
int haff_upscale_mask(const void* up1, const float* ln_w, const float* ln_b, const float* w2, const float* b2,
                      const float* hyper, float* out, int n_prompts, int h, int w, float eps, int dtype, void* stream);
/* F.interpolate(bilinear, align_corners=False) of the top-left [Hc][Wc] crop of in [N][Hs][Ws] -> out [N][Ho][Wo]
 * (both stages of Sam.postprocess_masks, sam.py:177-188) */
int haff_resize_bilinear(const float* in, float* out, int N, int Hs, int Ws, int Hc, int Wc, int Ho, int Wo,
                         void* stream);
/* ---- device-side frame ingest: the host resizes of the reference (Pillow, on uint8 RGB) and CLIP's normalisation ----
 * One axis of Pillow's antialiased resampling, bit-exact with Image.resize(BILINEAR|BICUBIC): replaces
 * ResizeLongestSide.apply_image (segment_anything/utils/transforms.py:27-34) and the resize inside
 * CLIPImageProcessor.preprocess (third-party transformers; call sites inference.py:233-236, utils/aff_dataset.py:76,228).
 * in u8 [B][Hin][Win][3] -> out u8 [B][Hout][Wout][3]; axis 0 resamples W (Hout == Hin), axis 1 resamples H (Wout == Win);
 * bounds i32 [n_out][2] (first input index, tap count) and coeffs i32 [n_out][ksize] (22-bit fixed point) are DEVICE tables
 * built by preprocess.pil_resample_tables. Horizontal pass first, then vertical. */
int haff_resample_u8(const void* in, void* out, int B, int Hin, int Win, int Hout, int Wout, int axis, const int* bounds,
                     const int* coeffs, int ksize, void* stream);
/* centre crop + 1/255 + (x-mean)/std of CLIPImageProcessor as a f32 [3][256] DEVICE lut: u8 NHWC window (top,left,S,S)
 * -> out [B][3][S][S], out_dtype 0 bf16 / 1 f32 (the images_clip argument of LISAForCausalLM.evaluate, LISA.py:432) */
int haff_clip_normalize_u8(const void* in, void* out, int B, int Hin, int Win, int top, int left, int S, const float* lut,
                           int out_dtype, void* stream);
/* Ground-truth masks of the fine-tune loader on the device: cv2.drawContours(mask, [contour], -1, 1, thickness=FILLED) per contour
 * (utils/aff_dataset.py:340-346) for a batch of planes in one call, byte for byte what cvlite.draw_contours_filled gives: the
 * 8-connected Bresenham outline of every edge (closing edge included, from the smaller-x end, clipped per pixel), then the 16.16
 * fixed-point scanline fill with crossings paired in x order WITHIN one polygon. out u8 [n_planes][H][W] holds 0 / 1.
 * ZEROING `out` IS PART OF THE CALL (a memset on `stream` in front of the kernels): the caller hands over any buffer.
 * pts i32 [n_pts][2] (x, y), poly_off i32 [n_poly + 1] (poly_off[0] == 0, non-decreasing, n_pts = poly_off[n_poly]) and poly_plane
 * i32 [n_poly] (the output plane of each polygon) are HOST arrays: they are checked here and never read by a kernel. desc_dev is the
 * caller's DEVICE copy of the same values, i32 [poly_off | poly_plane | pts] back to back, uploaded in stream order before the call.
 * Limits, all checked on the host copy before anything is enqueued: at most 4096 vertices per polygon, every |coordinate| < 32768,
 * H, W <= 32768, planes in range. Beyond them HAFF_ERR_BAD_ARG, and nothing is launched or zeroed. Within them no input can fail on
 * the device: the per-row crossing list lives in LDS sized by the launch's longest polygon. n_poly == 0 only zeroes. */
int haff_fill_contours_u8(const int* pts, const int* poly_off, const int* poly_plane, const int* desc_dev, int n_poly, int n_planes,
                          void* out, int H, int W, void* stream);
/* ---- training augmentation on the device (train_ds.py --aug_flip / --aug_jitter; csrc/frame_augment.hip): the offline
 * augmentations of the 2HANDS training set (2HANDS/scripts/data_augmentation/horizontal_flip.py, apply_jitter.py) per sample, byte
 * for byte what Pillow gives. frames u8 [B][H][W][3] at any address; flags i32 [B] (bit 0 mirror left-right, bit 1 colour jitter),
 * factors f32 [B][3] (brightness, contrast, colour; read only where bit 1 is set) and sums u64 [B] are DEVICE arrays.
 *   L(r,g,b)       = (19595 r + 38470 g + 7471 b + 32768) >> 16
 *   blend(d, i, f) = clip8(trunc(fl32(fl32(d) + fl32(f * fl32(i - d)))))   product and sum rounded separately, as Image.blend
 *   p1 = blend(0, p, fb);  S = sum of L(p1) over the frame, m = (2 S + H W) div (2 H W);  p2 = blend(m, p1, fc);
 *   p3 = blend(L(p2), p2, fs)   = ImageEnhance.Brightness(im).enhance(fb) -> Contrast(..).enhance(fc) -> Color(..).enhance(fs)
 * haff_jitter_stats_u8 writes S into sums[b] for every frame with bit 1 set and 0 for the others: the B slots are zeroed by the call
 * itself (a memset on `stream` in front of the kernel) and the partial sums are integers, so repeat runs are bitwise equal.
 * haff_augment_u8 is out of place and one pass: jitter (with sums as haff_jitter_stats_u8 left them for the same frames, flags and
 * factors) and / or Image.transpose(FLIP_LEFT_RIGHT) per frame; a frame with neither bit is copied.
 * haff_flip_planes_u8 mirrors the planes of u8 [P][H][W] whose flags[p] has bit 0 set and copies the others (the filled masks).
 * Refused before anything is enqueued: -1 for a NULL pointer, flags or factors not 4-B aligned, sums not 8-B aligned, a size <= 0,
 * out overlapping in (out == in included); -2 for H * W > 2^24 pixels in the two frame entry points (the caller augments such a
 * frame on the host). */
int haff_jitter_stats_u8(const void* frames, int B, int H, int W, const int* flags, const float* factors, void* sums, void* stream);
int haff_augment_u8(const void* in, void* out, int B, int H, int W, const int* flags, const float* factors, const void* sums,
                    void* stream);
int haff_flip_planes_u8(const void* in, void* out, int P, int H, int W, const int* flags, void* stream);
/* ---- the object-crop augmentation on the device (train_ds.py --aug_crop; csrc/frame_crop.hip): crop_and_pad of
 * 2HANDS/scripts/data_augmentation/process_cropped_sequences.py per sample, byte for byte what Pillow gives. in / out u8
 * [B][H][W][C], C = 3 (frames) or 1 (mask planes: v != 0 is read as 255, result != 0 is written as 1), out of place. The descriptor
 * is ONE int32 array given twice, as the host copy the call checks and as the device copy the kernel reads:
 *   words [12 b, 12 b + 12): x0 y0 cw ch px py S flags | htab hks vtab vks        flags: bit 0 mirror, bit 2 crop
 *   htab / vtab: word offsets of the sample's tables for S -> W and S -> H (preprocess.pil_resample_tables, bicubic), W resp. H rows
 *   of 2 + hks resp. 2 + vks words: (first input index, tap count, 22-bit coefficients). Samples with one S share their tables.
 *   Q[sy][sx] = src[y0 + sy - py][x0 + sx - px] inside the cw x ch window pasted at (px, py) on a black S x S square, S = max(cw, ch);
 *   out = Q.resize((W, H), BICUBIC): horizontal pass, uint8 intermediate (kept in LDS per output tile), vertical pass.
 * With bit 0 src is the sample with every row reversed (the box is the mirrored sample's); without bit 2 the sample is copied
 * (mirrored with bit 0) and the rest of its row is not read.
 * Refused before anything is enqueued: -1 for a NULL or misaligned pointer, a size <= 0, C other than 1 or 3, out overlapping in, a
 * box outside the sample, S != max(cw, ch), a paste outside the square, a table outside the descriptor or a table row outside
 * [0, S); -2 for H * W > 2^24, S > 4 W or S > 4 H (more than 17 taps), or a tile of 16 output rows reaching more than 96 source rows
 * (the caller crops such a sample on the host). */
int haff_crop_resample_u8(const void* in, void* out, int B, int H, int W, int C, const int* desc_host, const int* desc_dev,
                          long desc_words, void* stream);
/* mask > logit_th -> 0/255 bytes (inference.py:294-301 with logit_th = logit(th); chat.py:226 with 0) */
int haff_threshold_masks(const float* in, void* out, long total, float logit_th, void* stream);
/* a15 in one pass — the output gating + thresholds of 2Haff/inference.py:276-334 and chat.py:226-253:
 * planes[t][i] = (argmax(taxonomy) != blank_class && logits[i] > thresholds_host[t]) ? on_value : 0.
 * logits f32 [total] (16-B aligned), planes u8 [n_th][plane_stride] (plane_stride >= total, % 4 == 0), thresholds_host = HOST array of n_th <= 8 LOGIT thresholds
 * (sigmoid(m) > th restated as m > x*(th), exact in f32: 2handedafforder_amd/postprocess.py), taxonomy = DEVICE pointer
 * to the prompt's 4 class probabilities (argmax ties -> first, as torch.argmax) or NULL = gate open; blank_class 1 for the
 * left hand, 0 for the right (inference.py:278,305; chat.py:233,243). on_value 255 (inference PNGs) / 100 (chat JPGs). */
int haff_gate_threshold_masks(const float* logits, void* planes, long total, long plane_stride,
                              const float* thresholds_host, int n_th, int on_value, const float* taxonomy, int blank_class,
                              void* stream);
/* ---- the robot loop's per-request outputs (2Haff/robot_demo.py:57-73,266-327; csrc/robot_post.hip) ----
 * create_heatmap of n f32 logit planes [n][H][W] (4-B aligned; 16-B aligned with W % 4 == 0 takes the float4 path) -> out u8
 * [n][H][W][3] in RGB order: min-max normalisation to 0..255 as cv2.normalize (scale and shift in double, fmaf in float),
 * truncation, JET through jet_rgb (u8 [256][3]), the 5x5 sigma-1 Gaussian blur of OpenCV's bit-exact 8-bit path
 * (BORDER_REFLECT_101). workspace: workspace_floats >= n * 512 floats of scratch for the per-plane min / max partials (no
 * atomics: deterministic). */
int haff_robot_heatmap(const float* logits, int n, int H, int W, const void* jet_rgb, float* workspace, long workspace_floats,
                       void* out, void* stream);
/* logits f32 [H0][W0] -> out u8 [H0+top+bottom][W0+left+right] (4-B aligned): (logits > th) pasted at (left, top) (negative
 * margins crop, as PIL's paste), ANDed with the lowest bit of mask (u8 [mask_h][mask_w], 4-B aligned, or NULL = no AND), times
 * on_value. -1 when mask's size is not the padded size (cv2.bitwise_and raises) or the padded size is empty. */
int haff_robot_mask(const float* logits, int H0, int W0, int left, int top, int right, int bottom, float th, const void* mask,
                    int mask_h, int mask_w, int on_value, void* out, void* stream);
/* ---- the benchmark workflow's mask smoothing (ActAffordance/scripts/utils/gaussian.py: cv2.GaussianBlur(img, (7, 7), 0), then
 * `blurred / 255.0 > tau`; csrc/mask_smooth.hip) on the f32 logits, for every threshold at once ----
 * n contiguous f32 planes logits [n][H][W] -> out [n][H][W] (out != logits): every output is the weighted upper quantile of the
 * pixel's 49 taps under BORDER_REFLECT_101 (any overshoot; a side of 1 maps every tap to index 0), weights c[dy] c[dx] with
 * c = {8, 28, 56, 72, 56, 28, 8} (OpenCV's 7-tap table times 256; total 65536): the largest tap value v with
 * weight{taps >= v} >= need, need in 1..65536. The output is one of the inputs, bit for bit (but -0.0 and +0.0 compare equal and
 * either may be returned). A NaN tap counts as -inf; a pixel whose weight of taps above -inf is below need gets -inf; no NaN is
 * written. For a 0/255 plane p = 255 [logits > lt] of ANY lt, 255 [out > lt] is the 8-bit bit-exact blur of p followed by
 * `blurred / 255.0 > tau` when need = ceil((65536 b - 32768) / 255), b = min{b in 0..255 : b / 255.0 > tau} (tau = 0.5: 32768).
 * Both pointers 4-B aligned; a 16-B aligned logits with W % 4 == 0 takes the float4 path. One launch, no atomics, no workspace:
 * deterministic. -1 for a NULL or misaligned pointer, out == logits, n < 1, a side < 1, need outside 1..65536; -2 for a side over
 * 4096; nothing is written in either case. */
int haff_mask_quantile7(const float* logits, int n, int H, int W, int need, float* out, void* stream);
/* ---- benchmark scoring and validation metrics on the device (calculate_iou.py:117-337 as evaluation.py restates it,
 * 2Haff/train_ds.py:625-796; csrc/mask_score.hip) ----
 * One frame of a haff_score_masks batch: 128 bytes, every pointer a DEVICE pointer. */
typedef struct haff_score_frame {
  const float* logit[2];          /* left, right hand: f32 [Hs][Ws] mask logits as evaluate() returns them; NULL = hand missing */
  const float* taxonomy;          /* n_tax = 4 n class probabilities of the frame's n prompts, flattened; NULL = gated by the caller */
  const unsigned char* gt[2];     /* left, right ground truth: u8 [Hb][Wb], on where > 0; NULL = empty (calculate_iou.py:237-255) */
  const unsigned char* obj[2];    /* left, right object mask: u8 [Hb][Wb]; the hand counts only where obj > 0; NULL = no AND */
  unsigned char* out;             /* u8 [T][Hb][Wb]: the predicted two-hand union per threshold, 0/1; NULL = not written */
  int Hs, Ws, Hb, Wb, n_tax;
  int gt_hw[2][2], obj_hw[2][2];  /* (rows, columns) of each gt / obj plane as the caller holds it: checked against (Hb, Wb) */
  int vis;                        /* 0 = nothing drawn; k in 1..n_frames = record n_frames + k - 1 of the SAME tables, a haff_score_vis */
  int pad[2];
} haff_score_frame;
/* One overlay record of a haff_score_masks batch (calculate_iou.py:43-95, create_overlay): 128 bytes, every pointer a DEVICE pointer.
 * It sits behind the n_frames frame descriptors of the host and the device table; the frame whose vis names it supplies the logits,
 * gate, planes and (Hb, Wb). Per frame pixel (y, x): the target pixel is (row[y], col[x]) (clamped into the target grid); a hand's
 * prediction layer is on where the scoring rule above turns the hand on at threshold t (gate, resample, obj AND), its benchmark layer
 * where gt > 0; per channel c, in fp32 with every product and sum rounded on its own (never fused),
 * t1 = rgb * alpha[0] + (L ? color[0][c] : 0) * beta[0] + gamma,
 * u1 = saturate(round-half-even(t1)), t2 = u1 * alpha[1] + (R ? color[1][c] : 0) * beta[1] + gamma, byte = saturate(round-half-even(t2)):
 * two cv2.addWeighted calls on uint8. Both blends always run. out[0] takes the benchmark layers, out[1] the prediction layers. */
typedef struct haff_score_vis {
  const unsigned char* rgb;       /* u8 [Hf][Wf][3]: the frame as loaded (RGB) */
  const int* row;                 /* int32 [Hf]: nearest source row in the target grid (Hb, Wb) of every frame row */
  const int* col;                 /* int32 [Wf]: the same for columns; row and col both NULL = identity, needs (Hf, Wf) == (Hb, Wb) */
  unsigned char* out[2];          /* benchmark overlay, prediction overlay: pixel (y, x) at out[k] + y * stride[k] + 3 x; NULL = not drawn */
  long stride[2];                 /* bytes per canvas row, >= 3 Wf. Side by side: one canvas [Hf][2 Wf][3], out[1] = out[0] + 3 Wf, both 6 Wf */
  int Hf, Wf;
  int t;                          /* index of the threshold that is drawn */
  float alpha[2], beta[2], gamma; /* create_overlay: (0.5, 1), (0.5, 0.5), 0: every product and sum exact in fp32 */
  int color[2][3];                /* RGB of the left and the right hand, 0..255: (255, 0, 0) and (0, 255, 0) */
  int pad[4];
} haff_score_vis;
/* counts u32 [n_frames][n_th][4] = {intersection, union, predicted area, ground-truth area} of the two-hand unions of every frame
 * and LOGIT threshold, zeroed by the call itself (a kernel in front of the scoring launch, same stream), then one launch over
 * grid (blocks per frame, frames). Per target pixel and hand: the bilinear resample (half-pixel centres, no antialiasing) of the
 * 0/255 plane `logit > th` from (Hs, Ws) to (Hb, Wb) followed by `> 0`, in exact integers: per axis
 * num = max((2o+1) n_in - n_out, 0), i0 = min(num / 2 n_out, n_in - 1), i1 = min(i0 + 1, n_in - 1), w1 = num mod 2 n_out (0 when
 * i1 == i0), w0 = 2 n_out - w1; S = sum of wy wx [logit(tap) > th]; on iff 510 S > 4 Hb Wb. Strict compares: a NaN logit is off.
 * Equal sizes are the identity. Then AND with obj > 0, then the OR of the hands. Gate: argmax of taxonomy[0 .. n_tax) (first
 * maximum); index 1 blanks the left hand, index 0 the right one, any other neither. Integer atomics only: repeat runs are bitwise
 * equal. frames_host is the HOST copy of the n_frames descriptors, checked here and never read by a kernel; frames_dev the caller's
 * DEVICE copy, uploaded in stream order before the call. thresholds_host: HOST array of n_th floats.
 * When any frame has vis != 0 a third launch follows the scoring launch, grid (blocks, max vis), 256 threads, four consecutive
 * pixels of a frame row per thread, word stores where the canvas row allows and bytes otherwise, no atomics and no workspace: the
 * overlays of haff_score_vis, from the same per-pixel decisions that were counted. Both tables then hold n_frames + max(vis) records.
 * Refused before anything is enqueued: -1 for n_th outside 1..8, n_frames outside 1..65535, a side <= 0, a gt / obj plane whose
 * shape is not (Hb, Wb), n_tax outside 1..1024 with a taxonomy, a logit or taxonomy pointer that is not 4-B aligned, a descriptor
 * table that is not 8-B aligned, counts not 4-B aligned, a NULL table, thresholds or counts; -2 for a side over 4096. The u8
 * planes may sit at any address (4-B aligned quads move as words, the rest as bytes). After a frame's own checks, when its vis != 0:
 * -1 for vis outside 1..n_frames or named by an earlier frame too, a NULL rgb, both out NULL, only one of row / col, no tables with
 * (Hf, Wf) != (Hb, Wb), a row / col that is not 4-B aligned, t outside 0..n_th-1, a stride of a drawn canvas below 3 Wf, Hf < 1 or
 * Wf < 1; -2 for Hf or Wf over 4096. rgb and the canvases may sit at any address. Nothing is launched on a refusal. */
int haff_score_masks(const void* frames_host, const void* frames_dev, int n_frames, const float* thresholds_host, int n_th,
                     void* counts, void* stream);
/* ---- the benchmark's Hausdorff distances on the device (calculate_iou.py:9-24 as evaluation.calculate_hausdorff and
 * cvlite.find_contours_external restate it; csrc/contour_hausdorff.hip) ----
 * One plane of a haff_contour_hausdorff batch: 16 bytes, `plane` a DEVICE pointer to u8 [H][W] at any address, on where != 0. */
typedef struct haff_contour_plane {
  const unsigned char* plane;
  int H, W;
} haff_contour_plane;
/* For every plane: the CHAIN_APPROX_SIMPLE vertices of cv2.findContours(plane, RETR_EXTERNAL, CHAIN_APPROX_SIMPLE)[0] as cvlite
 * restates it. The plane is read inside one ring of background; foreground is 8-connected, background 4-connected; "outside" is
 * the background component of the ring; an 8-connected foreground component is external when one of its pixels has an outside
 * left neighbour; [0] is the outer border of the external component whose raster-first pixel comes LAST, followed from that pixel
 * as cvlite._follow does. For every pair (bench plane, pred plane), by index into the plane table (a frame of T thresholds is T + 1
 * planes and T pairs: the ground truth is walked once): d2(A -> B) = max over a in A of min over b in B of |a - b|^2 on the two
 * vertex lists, in integers. The caller takes the square roots and applies calculate_hausdorff's two empty rules.
 *   result     u32 [n_pairs][6] = {bench vertices, pred vertices, d2(pred -> bench), d2(bench -> pred), flags, 0}, every word
 *              written by the call. flags: bit 0 bench overflow (more than max_vertices vertices; the count is still the walk's
 *              full count), bit 1 bench fault (a bound of the labelling or of the walk, 8 H W + 8 steps, was reached: no input
 *              should), bits 2 and 3 the same for pred. A pair with a flag set or an empty side has both d2 fields 0.
 *   verts_out  NULL, or i16 [n_planes][max_vertices][2] (x, y) in walk order followed by i32 [n_planes] vertex counts; entries
 *              past a plane's count are left as they were. Without it the lists live in the workspace.
 *   workspace  workspace_bytes >= what haff_contour_hausdorff_workspace answers for the same planes and max_vertices, 16-B aligned.
 * planes_host / pairs_host are the HOST copies of the tables (pairs: int [n_pairs][2]), checked here and never read by a kernel;
 * planes_dev / pairs_dev the caller's DEVICE copies, uploaded in stream order before the call. Six launches on `stream`, integer
 * atomics on order-independent values only: repeat runs are bitwise equal.
 * Refused before anything is enqueued: -1 for a NULL table, workspace or result, n_planes outside 1..4096, n_pairs outside
 * 1..65535, a side <= 0, max_vertices outside 1..2^22, a workspace that is too small or not 16-B aligned, a plane table that is
 * not 8-B aligned, pairs, result or verts_out not 4-B aligned, a pair index outside the plane table, a pair whose two planes differ
 * in shape; -2 for a side over 4096 (coordinates are int16, d2 <= 2 * 4095^2). */
int haff_contour_hausdorff(const void* planes_host, const void* planes_dev, int n_planes, const int* pairs_host, const int* pairs_dev,
                           int n_pairs, int max_vertices, void* workspace, long workspace_bytes, void* verts_out, void* result,
                           void* stream);
/* Host only: *bytes_out = the workspace haff_contour_hausdorff needs for these planes (only H and W are read) and max_vertices.
 * The same refusals for the plane table and max_vertices; -1 for a NULL bytes_out. */
int haff_contour_hausdorff_workspace(const void* planes_host, int n_planes, int max_vertices, long* bytes_out);
/* ---- predictions as 2HANDS contour records (2HANDS/scripts/utils/compress_masks_to_json.py:60-92: cv2.findContours(mask,
 * RETR_EXTERNAL, CHAIN_APPROX_SIMPLE), every contour kept; cvlite.find_contours_external restates it) ----
 * For every plane of the same descriptor table as haff_contour_hausdorff: ALL external contours. A contour starts at every
 * foreground pixel that is the raster-first pixel of its 8-connected component and has x == 0 or a left neighbour in the outside
 * background; contours are ordered by DESCENDING raster index of that pixel (OpenCV's order) and each is followed from it as
 * cvlite._follow does. max_contours and max_vertices are per plane.
 *   verts    i16 [n_planes][max_vertices][2] (x, y): the contours back to back.
 *   offsets  i32 [n_planes][max_contours + 1]: entry k the first vertex of contour k, entry n_contours the total.
 *   summary  i32 [n_planes][4] = {n_contours, n_vertices, flags, 0}, every word written by the call. n_contours is always the true
 *            number; n_vertices the true total whenever n_contours <= max_contours. flags: 1 more vertices than max_vertices,
 *            2 fault (a bound of the labelling or of a walk was reached: no input should), 4 more contours than max_contours
 *            (then no contour is walked: n_vertices is 0 and bit 0 stays clear).
 *            With a flag set the plane's verts and offsets hold nothing of use and the caller recomputes the plane on the host.
 * Nothing outside a plane's own rows is written, and inside them nothing past n_vertices vertices and n_contours + 1 offsets.
 * Nine launches on `stream` (the labelling's four, start marks, numbering, a counting walk, the offsets' scan, the writing walk),
 * each ordered after the last by the stream alone; nothing is read back; repeat runs are bitwise equal.
 * Refused before anything is enqueued: what haff_contour_hausdorff refuses for the plane table, max_vertices and the workspace
 * (sized by haff_contour_extract_workspace); -1 for max_contours outside 1..2^22, a NULL verts, offsets or summary, or one that
 * is not 4-B aligned; -2 for a side over 4096. */
int haff_contour_extract(const void* planes_host, const void* planes_dev, int n_planes, int max_contours, int max_vertices,
                         void* workspace, long workspace_bytes, void* verts, void* offsets, void* summary, void* stream);
/* Host only: *bytes_out = the workspace haff_contour_extract needs. The same refusals for the plane table, max_contours and
 * max_vertices; -1 for a NULL bytes_out. */
int haff_contour_extract_workspace(const void* planes_host, int n_planes, int max_contours, int max_vertices, long* bytes_out);
/* ---- 2HANDS records from hand and object masks (2HANDS/scripts/affordance_extraction_preparation.py:256-304: pad_image,
 * cv2.resize(INTER_NEAREST), cv2.bitwise_and, delete_empty_masks, cv2.dilate, recolor_masks_white, as cvlite.extract_affordance and
 * cvlite.process_affordance restate them; csrc/affordance_extract.hip) ----
 * One item of a haff_affordance_extract batch: 64 bytes, every pointer a DEVICE pointer. */
typedef struct haff_extract_item {
  const unsigned char* in;        /* u8 [H][W] at any address: the completed mask, or any plane to process */
  const unsigned char* hand;      /* u8 [Hh][Wh] at any address; NULL = no AND */
  const int* col;                 /* i32 [W]: the hand's source column of every column, -1 (or anything outside 0..Wh-1) = padding */
  const int* row;                 /* i32 [H]: the same for rows; both tables are read only with a hand and may be shared by items */
  unsigned char* out;             /* u8 [H][W] at any address, not `in`; NULL = statistics only */
  int H, W, Hh, Wh;
  int pad[2];
} haff_extract_item;
/* a(y, x) = in(y, x) & hand[row[y]][col[x]], BITWISE as cv2.bitwise_and (1 & 2 = 0), 0 where either index is padding; in(y, x)
 * without a hand. out(y, x) = 255 when any a(y', x') != 0 with x' in [x - k/2, x + k - 1 - k/2] and y' in [y - k/2, y + k - 1 - k/2]
 * inside the image, else 0: cv2.dilate with np.ones((k, k)), the default anchor (k/2, k/2) and the default border, which keeps
 * taps outside the image out of the maximum, followed by recolor_masks_white. For even k the window is not symmetric: a lone pixel
 * at column 5 turns on columns 4..7 for k = 4, one at column 0 columns 0..2. k = 1 is the recolour alone.
 *   stats  i64 [n_items][8], every word written by the call (a kernel in front of the main launch, same stream):
 *          {non-zero pixels of a (delete_empty_masks' test, BEFORE the dilation), non-zero pixels of out, sum of the values of a,
 *           min row, max row, min column, max column of out's on pixels (H, -1, W, -1 for an empty plane), flags}.
 *          flags: 1 a hand was ANDed in, 2 a holds a value other than 0 and 255 (its sum / 255 is then no pixel count).
 * Two launches over grid (16 x 64 tiles of the largest item, items); integer atomics on order-independent values only: repeat runs
 * are bitwise equal. items_host is the HOST copy of the descriptors, checked here and never read by a kernel; items_dev the
 * caller's DEVICE copy, uploaded in stream order before the call. The tables' lengths are the caller's to check; their values are
 * bounds-checked by the kernel.
 * Refused before anything is enqueued: -1 for a NULL table or stats, one that is not 8-B aligned, n_items outside 1..65535, a NULL
 * in, out == in, a side <= 0, a hand without both tables or with one that is not 4-B aligned; -2 for k outside 1..31 or a side
 * (of the plane or the hand) over 4096. */
int haff_affordance_extract(const void* items_host, const void* items_dev, int n_items, int k, void* stats, void* stream);


/* ==== training path (LoRA fine-tune: train_ds.py:489-622 driving model_forward, LISA.py:175-430) ==================
 * Contractions of the backward pass reuse the GEMM kernels: dX = dY.W (NT GEMM on a transposed weight copy),
 * dW = dY^T.X (NT GEMM on transposed operands), attention-shaped products over (batch, head) through the batched
 * entry points. z = zo*nb_inner + zi selects operand base + zo*s?o + zi*s?i (elements). */
int haff_gemm_bf16_batched(const void* A, long lda, long sAo, long sAi, const void* W, long ldw, long sWo, long sWi,
                           void* C, long ldc, long sCo, long sCi, int nb_outer, int nb_inner, int M, int N, int K,
                           int out_f32, void* stream);
/* fp16 fine-tuning: A, W and a 16-bit C IEEE binary16 */
int haff_gemm_f16_batched(const void* A, long lda, long sAo, long sAi, const void* W, long ldw, long sWo, long sWi,
                          void* C, long ldc, long sCo, long sCi, int nb_outer, int nb_inner, int M, int N, int K,
                          int out_f32, void* stream);
int haff_gemm_f32_batched(const float* A, long lda, long sAo, long sAi, const float* W, long ldw, long sWo, long sWi,
                          float* C, long ldc, long sCo, long sCi, int nb_outer, int nb_inner, int M, int N, int K,
                          void* stream);
/* batched transpose: in [z][R][ld_in] (C valid columns) -> out [z][Cp][Rp] contiguous, zero padded */
int haff_transpose(const void* in, long ld_in, long s_in_o, long s_in_i, void* out, int R, int C, int Rp, int Cp,
                   int nb_outer, int nb_inner, int dtype, void* stream);
/* activation forward / adjoint (dx = dy * act'(x)); SwiGLU on the interleaved [gate x16 | up x16] layout */
int haff_act_fwd(const void* x, void* y, long n, int act, int dtype, void* stream);
int haff_act_bwd(const void* x, const void* dy, void* dx, long n, int act, int dtype, void* stream);
int haff_swiglu_fwd(const void* gu, void* y, long M, int F, int dtype, void* stream);
int haff_swiglu_bwd(const void* gu, const void* dy, void* dgu, long M, int F, int dtype, void* stream);
/* out = alpha*a + beta*b (b may be null) */
int haff_axpby(const void* a, const void* b, void* out, long n, float alpha, float beta, int dtype, void* stream);
/* ---- ordered reductions of the fine-tune step: no atomics, bitwise repeatable for a given launch geometry (round 4). Each
 * producer writes per-block partial sums into a caller-provided DEVICE fp32 buffer; haff_reduce_partials adds them in index
 * order: out[j] (+)= sum_{p < n_parts} partials[(j / out_inner) * group_stride + p * part_stride + j % out_inner].
 * Replaces the atomic forms haff_sumsq / haff_mask_loss_stats / haff_colsum / haff_scatter_add_rows inside train_ops / autograd
 * (global gradient norm of train_ds.py:381, the loss sums of LISA.py:16-59, bias gradients, the embedding gradient). ---- */
int haff_reduce_partials(const float* partials, float* out, int n_out, int n_parts, int out_inner, long part_stride,
                         long group_stride, int accumulate, void* stream);
int haff_sumsq_partials(const void* g, float* partials /* >= 1024 */, long n, int dtype, int* n_parts, void* stream);
int haff_mask_loss_stats_partials(const float* x, const float* t, float* partials /* [n_samples][*n_parts][4], n_parts <= 256 */,
                                  int n_samples, long n, float wgt, int* n_parts, void* stream);
int haff_colsum_parts(long R);   /* row blocks haff_colsum_partials writes: partials is [parts][C] */
int haff_colsum_partials(const void* x, float* partials, long R, int C, int dtype, void* stream);
/* dE[id] += sum of the rows with that id, in the order of a STABLE sort (sorted_ids ascending, order = the permutation) */
int haff_scatter_add_rows_sorted(const long* sorted_ids, const long* order, const void* dx, float* dE, long rows, int C, int dtype,
                                 void* stream);
/* out[r][c] = a[r][c] * alpha[r * alpha_stride]: alpha fp32 in DEVICE memory, one scalar (alpha_stride 0) or one per row (1).
 * The upstream gradient of the loss nodes of LISA.py:414-422 (ce / taxonomy CE) applied in fp32 without a host read. */
int haff_scale_dev(const void* a, void* out, long rows, long cols, const float* alpha, long alpha_stride, int dtype, void* stream);
/* out = a * b elementwise (LoRA dropout mask) */
int haff_mul(const void* a, const void* b, void* out, long n, int dtype, void* stream);
/* LayerNorm (rms=0) / RMSNorm (rms=1) adjoint: dx; dyx (f32 [rows][C], may be null) = dy*xhat for the weight grad */
int haff_norm_bwd(const void* x, const void* dy, const float* w, void* dx, float* dyx, int rows, int C, float eps, int rms,
                  int dtype, void* stream);
/* the same with the residual branch's gradient folded in: x of a pre-norm block feeds the norm AND the residual add (transformers'
 * LlamaDecoderLayer; image_encoder.py:186-193), so dx = norm adjoint(dy) + add (add: same shape / dtype as x; dx may alias it). */
int haff_norm_bwd_add(const void* x, const void* dy, const float* w, const void* add, void* dx, float* dyx, int rows, int C,
                      float eps, int rms, int dtype, void* stream);
/* out[c] += sum_r x[r][c] (bias / norm-weight gradients); out f32, zeroed by the caller */
int haff_colsum(const void* x, float* out, long R, int C, int dtype, void* stream);
/* row softmax of scale*s (+ causal mask, row r = query r % Nq, key j visible iff j <= q + q_pos0) and its adjoint
 * dS = scale * P o (dP - rowsum(dP o P)); columns >= Nk are written as zeros (K-padding of the following GEMMs) */
int haff_softmax_fwd(const float* s, long ld, void* p, long ldp, long rows, int Nq, int Nk, float scale, int causal,
                     int q_pos0, int dtype, void* stream);
int haff_softmax_bwd(const void* p, long ldp, const float* dp, long ld, void* ds, long rows, int Nk, float scale, int dtype,
                     void* stream);
/* rotate-half RoPE on x [rows][H][d], position pos0 + row % Tlen; adjoint != 0 applies the transpose rotation */
int haff_rope(const void* x, long ldx, void* y, long ldy, const float* cos_sin, long rows, int Tlen, int H, int d, int pos0,
              int adjoint, int dtype, void* stream);
/* fused shift-free cross entropy: row_loss[r] = lse(logits[r]) - logits[r][labels[r]] (0 when labels[r] < 0);
 * dlogits (may be null) = (softmax - onehot) * gscale on valid rows (llava_llama.py:108-118 after the caller's shift) */
int haff_cross_entropy(const void* logits, long ld, const long* labels, float* row_loss, void* dlogits, long rows, int V,
                       float gscale, int dtype, void* stream);
/* per-sample mask losses (LISA.py:16-59) on f32 logits scaled by wgt: stats[s] = {bce_sum, sum(p*t), sum(p), sum(t)}
 * (zeroed by caller); grad: dx = wgt*(c_bce*(p-t)/n + c_dice*d dice/dz) */
int haff_mask_loss_stats(const float* x, const float* t, float* stats, int n_samples, long n, float wgt, void* stream);
int haff_mask_loss_grad(const float* x, const float* t, const float* stats, float* dx, int n_samples, long n, float wgt,
                        float c_bce, float c_dice, void* stream);
/* the same with the upstream gradients of {bce, dice} read from device memory (coef f32 [n_samples][2]): no host read-back */
int haff_mask_loss_grad_dev(const float* x, const float* t, const float* stats, float* dx, int n_samples, long n, float wgt,
                            const float* coef, void* stream);
/* taxonomy loss (LISA.py:414-417): CrossEntropyLoss on the already soft-maxed probabilities p = softmax(z) with a soft
 * target t: loss[r] = -sum_c t_c log_softmax(p)_c; probs / dz may be null; C <= 8 */
int haff_taxonomy_ce(const float* z, const float* t, float* probs, float* loss, float* dz, int rows, int C, void* stream);
/* adjoint of haff_resize_bilinear (din zeroed by caller) */
int haff_resize_bilinear_bwd(const float* dout, float* din, int N, int Hs, int Ws, int Hc, int Wc, int Ho, int Wo,
                             void* stream);
/* embedding gradient dE[ids[r]] += dx[r] (f32 accumulator; ids < 0 skipped) */
int haff_scatter_add_rows(const long* ids, const void* dx, float* dE, long rows, int C, int dtype, void* stream);
/* out += sum(g^2) (gradient-norm clipping, train_ds.py:370) */
int haff_sumsq(const void* g, float* out, long n, int dtype, void* stream);
/* fused AdamW on fp32 master weights (+ optional 16-bit copy), torch semantics, gradient pre-scaled by gscale.
 * g_dtype: 0 bf16 / 1 f32 / 3 f16 gradients; lp_dtype: -1 no copy, 0 bf16 copy, 3 f16 copy (= f16_rn(master)); other codes -1 */
int haff_adamw_step(float* master, float* m, float* v, const void* g, void* param_lp, long n, float lr, float beta1,
                    float beta2, float eps, float wd, int step, float gscale, int g_dtype, int lp_dtype, void* stream);
/* the same, the gradient scale multiplied by *gscale_dev (device f32: the clip coefficient computed on the device) */
int haff_adamw_step_dev(float* master, float* m, float* v, const void* g, void* param_lp, long n, float lr, float beta1,
                        float beta2, float eps, float wd, int step, float gscale, const float* gscale_dev, int g_dtype,
                        int lp_dtype, void* stream);
/* the fp16 mode's step: as haff_adamw_step_dev (gscale_dev may be null), skipped when the device gradient norm *norm is not finite
 * (an inf / NaN gradient element: loss-scale overflow) — master, m, v and the copy then keep every bit */
int haff_adamw_step_skip(float* master, float* m, float* v, const void* g, void* param_lp, long n, float lr, float beta1,
                         float beta2, float eps, float wd, int step, float gscale, const float* gscale_dev, const float* norm,
                         int g_dtype, int lp_dtype, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HAFF_HIP_H */
