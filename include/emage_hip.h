/*
 * emage_hip.h — C ABI of libemage_hip.so, the MI355X (gfx950) kernels behind the EMAGE hot path.
 *
 * The reference (PantoMatrix @ 2025-01-17) has no FFI/operator registry for this path: the
 * arithmetic lives in torch.nn calls made from
 *   models/emage_audio/modeling_emage_audio.py   (M:)
 *   models/emage_audio/processing_emage_audio.py (P:)
 * Each entry point below replaces one ATen op family at the cited call sites (SURVEY.md §2b K1-K11,
 * §8b last row).  Conventions, all entry points:
 *   - extern "C", plain device pointers + sizes, no torch types;
 *   - non-owning: never allocates, frees or synchronises; safe inside hipGraph capture;
 *   - `stream` is a hipStream_t passed as void*;
 *   - returns 0 on success, a hipError_t (> 0) from the launch, or a negative EMAGE_E* code for
 *     an argument the kernels do not support (the host turns non-zero into an exception);
 *   - activations are (B,T,C) row-major == (rows, C) with a row stride `ld*` in ELEMENTS;
 *   - `dtype` selects the storage/MFMA operand type of activations and weights:
 *       EMAGE_F32  : float32 operands, v_mfma_f32_16x16x4_f32  (exact fp32, parity mode)
 *       EMAGE_BF16 : bfloat16 operands, v_mfma_f32_16x16x32_bf16, fp32 accumulate
 *       EMAGE_F16X3: (emage_gemm only) float32 activations, weights pre-split into two fp16 planes; every
 *                    product runs as three v_mfma_f32_16x16x32_f16 (hi*hi + hi*lo + lo*hi, fp32 accumulate):
 *                    ~22 mantissa bits per product, i.e. fp32-grade results at 1/3 of the fp16 MFMA rate
 *                    instead of the 1/16 of the fp32 MFMA.  Every other entry point takes EMAGE_F32 tensors
 *                    in this mode (the storage type IS float32).
 *     accumulators, biases, LayerNorm statistics, softmax and every index are fp32 / int64 in
 *     all modes.
 */
#ifndef EMAGE_HIP_H
#define EMAGE_HIP_H

#include <stdint.h>

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EMAGE_F32 0
#define EMAGE_BF16 1
#define EMAGE_F16X3 2
#define EMAGE_H2 3
/* EMAGE_H2 with the activation scale of a MODEL: activation images (what emage_gemm / emage_layernorm / emage_attention / emage_add / emage_cast_pad /
 * emage_pack_motion / emage_gather_rows WRITE as `out`, and what emage_gemm / emage_add read as an H2 residual / operand) hold x * 2^(4 - k)
 * instead of 16 x: |x| < 4094 * 2^k stays finite in the fp16 hi plane, at the price of k bits of the smallest values' lo plane.  k = 0..12;
 * EMAGE_H2_SHIFT(0) == EMAGE_H2 (the default: bit-identical to the plain code).  emage_gemm's operand A is described by `a_scale` as before
 * (pass 2^(4 - k) for an activation image written under shift k); weight / gradient images (emage_h2_cast: explicit scale) are not affected. */
#define EMAGE_H2_SHIFT(k) (EMAGE_H2 | ((k) << 8))

#define EMAGE_EINVAL (-1)   /* unsupported size / alignment / null pointer */

/* Library identification: ABI version (bumped on any signature change) and target arch string. */
int emage_abi_version(void);
const char* emage_target_arch(void);

/*
 * Tools build only (libemage_hip_tools.so, compiled with -DEMAGE_TOOLS; the product library libemage_hip.so has neither this entry
 * point nor any other mutable global state).  Process-global, not thread-safe:
 *   key 0: force emage_gemm's tile configuration id of the F32 / BF16 / F16X3 modes (-1 restores the heuristic);
 *   key 1: diagnostic ablation mask for tools/bench_gemm.py --ablate (1 no operand DMA, 2 no MFMA, 4 no epilogue;
 *          8 / 16: write-through / non-temporal result stores, a recorded negative experiment);
 *   key 2: tile-heuristic variant for A/B runs;   key 3: timing ablations of emage_lstm_layer;
 *   key 4: force the EMAGE_H2 tile configuration id;   key 5: EMAGE_H2 tile-heuristic variant;   key 6: attention variant;
 *   key 7: EMAGE_H2 tile configuration for grids of at most one 64 x 64 tile per CU (0 = the shipped one);
 *   key 8: retired (it selected an antiphase EMAGE_H2 configuration).  Value 0 ("off") returns 0 so that callers which always set it
 *          keep working; any other value returns EMAGE_EINVAL.
 * Returns EMAGE_EINVAL for unknown keys.  emage_h2_set_trace: device buffer (waves x 512 uint64) for the phase tracer of the
 * instrumented EMAGE_H2 configurations (tools/trace_gemm_h2.py).
 */
#ifdef EMAGE_TOOLS
int emage_set_tuning(int key, int value);
int emage_h2_set_trace(void* buf);
#endif

/*
 * K6 — VQ nearest neighbour.  Replaces Quantizer.map2index / Quantizer.forward's argmin (P:144-164)
 * and EmageVQVAEConv.decode_from_latent's inline copy (M:60-67):
 *   d[n][k] = (sum_j z[n][j]^2 + sum_j e[k][j]^2) - 2 * sum_j z[n][j] e[k][j];  idx[n] = argmin_k d[n][k]
 * fp32 throughout, first minimum wins ties and a NaN distance wins outright (torch.argmin).  z: (N,D) fp32 row stride
 * ldz; codebook: (K,D) fp32 contiguous.  D % 4 == 0, D <= 1024, K <= 4096.
 * idx: int64, addressed as a 2-D view — element n is written at idx[(n / idx_rows) * idx_ld + n % idx_rows], so a
 * (B, T) window of a longer (B, L) code buffer is filled in place (idx_rows = T, idx_ld = L); idx_rows <= 0: a
 * plain (N,) list.  The same view convention is used by emage_argmax_logsoftmax_f32 (output) and emage_gather_rows
 * (input, with an extra frame stride idx_tstride in {0, 1}: 0 broadcasts one id per clip over its idx_rows frames).
 */
int emage_vq_argmin_f32(const float* z, int ldz, const float* codebook, int64_t* idx, int idx_rows, long idx_ld,
                        int N, int K, int D, void* stream);

/*
 * K8 — code selection from classifier logits.  Replaces torch.max(F.log_softmax(x, dim=2), dim=2)[1]
 * (M:398-401, test_emage_audio.py:39-42): y = (x - max) - log(sum exp(x - max)) in fp32, first maximum.
 * logits: (N,C) fp32 row stride ld; idx: (N,) int64.  C <= 4096.
 */
int emage_argmax_logsoftmax_f32(const float* logits, int ld, int64_t* idx, int idx_rows, long idx_ld, int N, int C, void* stream);

/*
 * K7 — codebook / embedding gather.  Replaces Quantizer.get_codebook_entry (P:166-170).
 * table: (K,D) fp32; idx: int64 view (see emage_vq_argmin_f32), clamped to [0, K); out: (N, ldo) in `dtype`,
 * columns [D, n_store) zero-filled.
 */
int emage_gather_rows(const float* table, const int64_t* idx, int idx_rows, long idx_ld, int idx_tstride,
                      void* out, int ldo, int n_store, int N, int K, int D, int dtype, void* stream);

/*
 * Quantizer.forward in TRAINING mode (P:144-156) behind emage_vq_argmin_f32, which stays the one place the codes are chosen.
 * z: (N, ldz) fp32 encoder output; codebook: (K, D) fp32 contiguous; idx: (N,) int64 contiguous (clamped to [0, K)).
 *   emage_vq_quantize_train writes zq (N, ldo) fp32 = codebook[idx[n]] and, when zq_image is non-NULL, the same rows as the decoder's
 *   operand image ((N, ld_image) in `dtype`: EMAGE_F32 / EMAGE_BF16 / EMAGE_H2, columns [D, n_store) zero, like emage_gather_rows);
 *   hist (K int32) = bincount(idx) (cleared by the call; integer atomics); scalars[0] = embedding_loss = (1 + beta) * mean((zq - z)^2),
 *   scalars[1] = perplexity = exp(-sum_k p_k log(p_k + 1e-10)), p = hist / N: float64 partial sums per 16-row block in `workspace`
 *   (emage_vq_quantize_train_workspace_bytes(N) bytes, 8-byte aligned), added in block order by a second one-block launch — no host
 *   read-back, no floating-point atomics.
 *   emage_vq_quantize_backward, with s = 2 / (N D) and g_loss ONE fp32 on the device (the gradient arriving at embedding_loss):
 *     dz[n] = g_zq[n] + g_loss * beta * s * (z[n] - e[idx[n]])      (g_zq (N, ldg): the straight-through gradient, may be NULL)
 *     d_codebook[k] = g_loss * s * sum_{n : idx[n] = k} (e[k] - z[n])  (K, D) contiguous, zero for unused codes; g_zq does not reach it
 *   One block per code scans idx and adds its rows in ascending n in float64: bit-reproducible run to run.
 */
long emage_vq_quantize_train_workspace_bytes(int N);
int emage_vq_quantize_train(const float* z, int ldz, const float* codebook, const int64_t* idx, float* zq, int ldo,
                            void* zq_image, int ld_image, int n_store, int dtype, int* hist, float* scalars, float beta,
                            void* workspace, long workspace_bytes, int N, int K, int D, void* stream);
int emage_vq_quantize_backward(const float* z, int ldz, const float* codebook, const int64_t* idx, const float* g_zq, int ldg,
                               const float* g_loss, float beta, float* dz, int ld_dz, float* d_codebook, int N, int K, int D,
                               void* stream);

/*
 * The gradient of an embedding table read one row per CLIP — the backward of emage_gather_rows(table, ids broadcast over T) with respect to
 * `table` (EmageAudioModel's two speaker tables, M:217-219 / 285-286; csrc/embedding.hip):
 *   dw[s][c] = sum over clips b with clamp(ids[b]) == s, b ascending, of sum over t < T, t ascending, of g[(b * T + t) * ldg + c]
 * g: (B * T, D) fp32 rows of pitch ldg >= D; ids: (B,) int64 contiguous, clamped exactly as emage_gather_rows clamps (below 0 -> 0, at or
 * above S -> S - 1: forward and backward agree on the row a clip used, and nothing is indexed with an unclamped id); dw: (S, D) fp32 rows
 * of pitch lddw >= D, WRITTEN (not accumulated): a row no clip names is 0.0f.  1 <= D <= 4096, 1 <= S <= 1024, B, T >= 1.
 * Sums are float64, rounded to fp32 once, in the fixed order above; no floating-point atomics: bit-reproducible run to run and replay to
 * replay.  workspace: emage_embedding_backward_workspace_bytes(B, D) = B * D * 8 bytes, 8-byte aligned, lent by the caller (the per-clip
 * sums of the first of the two launches); the library never allocates.
 */
long emage_embedding_backward_workspace_bytes(int B, int D);
int emage_embedding_backward(const float* g, long ldg, const int64_t* ids, int B, int T, int D, int S, float* dw, long lddw,
                             void* workspace, long workspace_bytes, void* stream);

/*
 * K1/K2/K3 — the one contraction kernel: Linear and Conv1d as (implicit) GEMM with a fused epilogue.
 * Replaces nn.Linear (M:232-263 call sites, MLP P:316-326), nn.Conv1d k=3 of VQEncoderV5/V6,
 * VQDecoderV5, ResBlock (P:178-261) and nn.Conv1d k=15 (+ folded eval BatchNorm1d + LeakyReLU +
 * shortcut add) of BasicBlock (P:263-294).
 *
 *   out[m][n] = leaky( sum_{tap,c} A[row(m,tap)][c] * W[n][tap*Cp + c] + bias[n], slope[n] ) + res[m][n]      (res_first = 0)
 *   out[m][n] = leaky( sum_{tap,c} ...                                + bias[n] + res[m][n], slope[n] )      (res_first = 1,
 *               BasicBlock's "x += shortcut; act2(x)", P:291-293)
 *   m = b*Lout + l,  row(m,tap) = b*Lin + l*stride + tap - pad, taken as zeros when
 *   l*stride + tap - pad is outside [0, Lin)   (taps=1,stride=1,pad=0,Lin=Lout => plain Linear).
 *   The formula holds for taps == 1 too: taps=1 with stride != 1, pad != 0 or Lin != Lout is a 1 x 1 convolution with that geometry, not a Linear.
 *   EMAGE_EINVAL: pad < 0, stride <= 0, Lin <= 0, Lout <= 0, M % Lout != 0 (checked before any launch); the LayerNorm fold of
 *   emage_gemm_problem needs the plain Linear geometry.
 *
 * A:     (rows_in, lda) `dtype`; channels [C, Cp) must hold finite values (they meet zero weights).
 * W:     (N, taps*Cp) `dtype`, Cp % 64 == 0, zero in the padded channels; K = taps*Cp.
 * bias:  (N) fp32 or NULL.   slope: (N) fp32 or NULL; leaky(v,s) = v > 0 ? v : v*s
 *        (0 = ReLU, 1 = identity, 0.2 / 0.1 / 0.01 = the reference's LeakyReLU slopes).
 * res:   (M, ldr) residual, fp32 if res_is_f32 else `dtype`; or NULL.
 * out:   (M, ldo) `dtype` or NULL; columns [N, n_store) are written as zeros (keeps padded channel
 *        tails finite for the next contraction).   out_f32: (M, ldf) fp32 or NULL.
 * out_t: transposed destination or NULL: columns n >= t_col0 go to out_t[(b*(N-t_col0) + n-t_col0)*t_ld + l]
 *        instead of `out` (b = m / t_rows, l = m % t_rows) — used to emit V^T for emage_attention.
 * EMAGE_F16X3: A / res / out / out_t are float32; W is the host-packed split image of (W * w_scale): per row and per
 *        32-k tile 128 bytes = [4 hi chunks | 4 lo chunks], chunk g = 8 fp16 for k = 4g..4g+3, 16+4g..16+4g+3 of the
 *        tile (hi = rne_f16(w*w_scale), lo = rne_f16(w*w_scale - hi)); A is multiplied by a_scale before its own
 *        split and the accumulators by 1/(a_scale*w_scale) after the K-loop — both scales are powers of two chosen so
 *        that the fp16 planes stay in the normal range (|A*a_scale| must stay below 65504).  Other dtypes ignore them.
 * EMAGE_H2:  A / out / (res_is_f32 = 0) res are pre-split images (csrc/h2.h: per 8 columns 32 bytes [8 fp16 hi | 8 fp16 lo] of 16 x),
 *        out_f32 / out_t float32; W is the same image of W * w_scale, rows K-contiguous.  res == out_f32 (fp32, ldr == ldf) accumulates:
 *        out_f32 += contraction (a weight gradient added straight into the parameter's gradient, loss.backward()'s accumulation T:174).
 *        A bare contraction (no bias / slope / out / out_t, no LayerNorm fold or st_out) with few tiles and K >= 2048 is cut into K-slices
 *        added with fp32 atomics.
 */
int emage_gemm(int dtype, const void* A, int lda, const void* W, const float* bias, const float* slope,
               const void* res, int ldr, int res_is_f32, int res_first,
               void* out, int ldo, int n_store, float* out_f32, int ldf,
               void* out_t, int t_col0, int t_rows, int t_ld,
               int M, int N, int Cp, int taps, int stride, int pad, int Lin, int Lout,
               float a_scale, float w_scale, void* stream);

/*
 * emage_gemm with a caller-owned WORKSPACE (round 5; the weight-gradient contractions of the training step, train_emage_audio.py:176
 * `loss.backward()`): same arguments, meaning and validation as emage_gemm, plus `workspace` — device memory, 16-byte aligned,
 * `workspace_bytes` long (NULL: exactly emage_gemm).  EMAGE_H2, bare contractions (only out_f32, optionally accumulating: res == out_f32) with
 * few tiles and K >= 2048: the contraction is cut into as many K-slices as fill the chip's block slots once; every slice stores its partial
 * tile as a plane of the workspace (plain stores) and a second launch adds the planes IN SLICE ORDER onto the destination — a fixed
 * association: the result is the same bits on every run, which the fp32-atomic form of emage_gemm is not.  The number of slices is limited
 * by the workspace (M * round_up(N, 4) * 4 bytes per slice); below two slices the call falls back to emage_gemm's behaviour.  The library
 * neither allocates nor keeps the workspace; its contents are scratch after the call.  Other dtypes / shapes ignore it.
 */
int emage_gemm_ws(int dtype, const void* A, int lda, const void* W, const float* bias, const float* slope,
                  const void* res, int ldr, int res_is_f32, int res_first,
                  void* out, int ldo, int n_store, float* out_f32, int ldf,
                  void* out_t, int t_col0, int t_rows, int t_ld,
                  int M, int N, int Cp, int taps, int stride, int pad, int Lin, int Lout,
                  float a_scale, float w_scale, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Several INDEPENDENT emage_gemm problems in as few launches as possible — the part-wise stacks of the model run the same shapes on
 * different weights side by side: the four VQ-VAE part decoders (M:126-193 -> P:237-261), the three refinement decoder layers and
 * their heads (M:248-263, 320-330), `motion2latent_{upper,hands,lower}.fc2` (M:315-317), the two `bodyhints_*` MLPs (M:232-233).
 * Each problem is one emage_gemm call (same fields, same meaning, same validation); the result is bit for bit that of issuing the
 * calls one by one.  No problem may read what another problem of the same call writes.  EMAGE_H2: problems that select the same tile
 * configuration share a launch (up to 8 per launch; a block finds its problem by a prefix sum over the problems' tile counts, then
 * runs the unchanged tile routine) — a stack of N = 256 problems that leaves most CUs with one 4-wave block each becomes one launch
 * with several resident blocks per CU.  Other dtypes: one launch per problem.
 */
typedef struct emage_gemm_problem {
    const void* A; const void* W; const float* bias; const float* slope; const void* res;
    void* out; float* out_f32; void* out_t;
    int lda, ldr, res_is_f32, res_first, ldo, n_store, ldf, t_col0, t_rows, t_ld;
    int M, N, Cp, taps, stride, pad, Lin, Lout;
    float a_scale, w_scale;
    /* LayerNorm FOLDED into the contractions around it (EMAGE_H2, taps = 1; every pointer NULL = off; emage_gemm itself never folds).
     * A post-norm transformer layer (nn.TransformerDecoderLayer, modeling_emage_audio.py:238-250) computes y = LN(s) W^T + b on the
     * pre-norm sum s of the previous sub-layer.  With W' = W gamma, c[n] = sum_k W'[n][k], b' = W beta + b (packed by the host):
     *     y[m][n] = rstd[m] ( (s W'^T)[m][n] - mu[m] c[n] ) + b'[n]
     * so the contraction runs on the RAW sum (A = the EMAGE_H2 image of s, W = W', bias = b') and no LayerNorm launch / normalised
     * tensor exists.  Row statistics travel as PARTIALS {mean, M2} (float pairs) over 32 columns each, written by the epilogue of the
     * launch that produced s (st_out) and merged (Chan) by every consumer:
     *   ln_stats (M, ln_np) pairs, ln_np * 32 == Cp, ln_np == 24 (the 768-wide residual stream; other widths are refused: EMAGE_EINVAL): statistics of A's rows;  ln_c (N): c;  ln_eps: the LayerNorm's eps;
     *   rs_stats (M, rs_np) pairs, rs_np * 32 == N: `res` (an EMAGE_H2 image, res_is_f32 = 0) is the raw sum s' of a folded LayerNorm,
     *       the residual added is (s' - mu) rstd rs_gamma[n] + rs_beta[n];
     *   st_out (M, N / 32) pairs: partial statistics of THIS launch's output rows (values as stored to out / out_f32); N % 64 == 0, no
     *       out_t, launches that take the 64 x 64 tile (N < 1024) only.
     * A launch with any of these is never cut into K-slices by the atomic or the two-pass split-K (the epilogue of a slice sees partial
     * sums only); the in-launch fix-up below runs its one epilogue on the summed tile. */
    const float* ln_stats; const float* ln_c; const float* rs_stats; const float* rs_gamma; const float* rs_beta; float* st_out;
    int ln_np, rs_np;
    float ln_eps;
    /* Split-K with an in-kernel fix-up (EMAGE_H2; optional, NULL = off): a launch of few rows (ONE clip: M = 64 — a dozen 64 x 64 tiles that
     * would each walk the whole K range alone on one CU) may be cut into K-slices when the caller lends it scratch memory: sk_ws (16-byte
     * aligned, sk_ws_bytes; 16 KiB per tile and slice) and sk_count (sk_tiles ints, ZERO on entry; the launch leaves them zero).  Every
     * block stores its partial accumulators write-through, the last block of a tile to arrive adds the slices in slice order (the same bits on
     * every run) and runs the ordinary epilogue.  The library decides per launch (<= 128 tiles, >= 8 K-tiles of 32, capacity); launches on
     * ONE stream may share the scratch, concurrent streams need their own. */
    void* sk_ws; long sk_ws_bytes; int* sk_count; int sk_tiles;
} emage_gemm_problem;
int emage_gemm_grouped(int dtype, const emage_gemm_problem* problems, int n_problems, void* stream);
/* Launches nothing: the number of kernel launches emage_gemm_grouped would make of these problems (> 0), or a negative EMAGE_E* code. */
int emage_gemm_grouped_launches(int dtype, const emage_gemm_problem* problems, int n_problems);

/*
 * K1 first layer — WavEncoder block 0 on the raw waveform (Cin = 1), P:301 + P:283-290:
 *   out[b][l][c] = leaky( sum_k wav[b][l*stride + k - pad] * w[c][k] + bias[c], slope[c] )
 * wav: fp32, clip b at wav + b*ldw; the launch covers `nwin` windows of L samples per clip, window i starting at
 * sample i*hop of its clip (inference()'s sliding windows, M:393-394, read in place: no slicing copy); samples
 * outside [0, L) of a window are the conv's zero padding.  Output sequence (i*B + b) holds window i of clip b:
 * out: (nwin*B*Lout, ldo) `dtype`.  w: (C, taps) fp32 (eval BatchNorm folded).
 * Computes conv1 and the downsample shortcut (same input, same geometry) in one pass: the host
 * stacks their filters along C and gives the shortcut channels slope 1.  C % 8 == 0, taps <= 16.
 */
int emage_wav_conv_in(int dtype, const float* wav, long ldw, int L, int nwin, long hop,
                      const float* w, const float* bias, const float* slope,
                      void* out, int ldo, int B, int Lout, int C, int taps, int stride, int pad, void* stream);

/*
 * The audio front end in one launch (what `librosa.load(path, sr=16000)` does for PCM input, test_emage_audio.py:17-18): decode, channel
 * mean and rational-rate polyphase low-pass resampling, out = scipy.signal.resample_poly(mean(decode(pcm)), up, down) in fp32.
 *   pcm:  n_clips clips of n_in interleaved frames of `channels` (1..8) samples, clip b at (char*)pcm + b * clip_pitch_bytes
 *         (>= one clip).  fmt: EMAGE_PCM_S16 (/ 32768), EMAGE_PCM_S24 (packed 3-byte little endian, sign-extended, / 8388608),
 *         EMAGE_PCM_S32 (int32 -> float32 round-to-nearest, / 2^31), EMAGE_PCM_F32.  16- and 32-bit samples at their natural alignment;
 *         16-bit mono / stereo with a 16-byte aligned base and pitch is read with 16-byte loads.
 *   mono: the fp32 sum of a frame's samples in channel order, divided by `channels` (one channel: the sample itself).
 *   out:  (n_clips, ldo >= n_out) fp32, n_out == ceil(n_in * up / down):
 *           out[b][m] = sum_k h[m * down + half - k * up] * mono[b][k],   half = 10 * max(up, down),  0 <= k < n_in,
 *         fp32 taps, fp32 accumulation with fused multiply-add, k descending.  One writer per output: bit-reproducible.
 *   taps: the n_taps == 2 * half + 1 filter taps h as PHASE ROWS, 16-byte aligned: `up` rows of pitch (rpp | 1) floats, rpp = ceil(n_taps / up);
 *         row p holds h[p], h[p + up], h[p + 2 up], ... and zeros up to the pitch (odd: with 32 | up and down odd, the rows 32 neighbouring
 *         lanes read start on 32 different LDS banks).  up == down == 1: decode and down-mix only, taps / n_taps are ignored.
 *   The padded taps of a short row are multiplied too (0 * x): with EMAGE_PCM_F32 an Inf / NaN sample within one row length of an output's
 *   window makes that output NaN where the exact sum would skip it; integer PCM cannot produce one.
 * LDS budget: the phase rows (up * (rpp | 1) * 4 bytes) must fit EMAGE_AUDIO_TAPS_LDS_BYTES, and the decoded input span of one tile of
 * EMAGE_AUDIO_TILE outputs (ceil((TILE - 1) * down / up) + rpp + 17 floats) EMAGE_AUDIO_SPAN_LDS_BYTES: together the 160 KiB of a CU.
 * 44 100 -> 16 000 Hz (8 821 taps) takes 36 KiB + 12 KiB, 11 025 -> 16 000 Hz (12 801 taps) 53 KiB + 3 KiB; down / up beyond about 15 is refused.
 * EMAGE_EINVAL: null pointers, unknown fmt, channels outside 1..8, n_out != ceil(n_in up / down), ldo < n_out, clip_pitch_bytes smaller
 * than a clip, n_taps != 20 max(up, down) + 1, a table or span beyond the budget, misaligned samples / taps, n_clips > 65535.
 */
#define EMAGE_PCM_S16 0
#define EMAGE_PCM_S24 1
#define EMAGE_PCM_S32 2
#define EMAGE_PCM_F32 3
#define EMAGE_AUDIO_TILE 1024
#define EMAGE_AUDIO_TAPS_LDS_BYTES (96 * 1024)
#define EMAGE_AUDIO_SPAN_LDS_BYTES (64 * 1024)
int emage_audio_resample(int fmt, const void* pcm, long clip_pitch_bytes, int channels, long n_in,
                         const float* taps, int n_taps, int up, int down,
                         float* out, long ldo, long n_out, int n_clips, void* stream);

/*
 * K1, LDS-resident input slab — the stride-1, k <= 16 convolutions with C == N in {64, 128} channels (BasicBlock conv2 of every
 * WavEncoder block and conv1 of the stride-1 blocks, P:263-306), same arithmetic as emage_gemm with taps = k, stride 1:
 *   out[s][l][n] = leaky( sum_{tap,c} A[s][l + tap - pad][c] * W[n][tap*C + c] + bias[n] + res[s][l][n], slope[n] )
 * A block owns 128 positions of one sequence: its 128 + k - 1 input rows are loaded into LDS ONCE (in EMAGE_F16X3 already
 * split into fp16 hi / lo planes) instead of once per tap, and only the W tiles stream through the LDS-DMA ring.
 * A: (nseq*L, lda) `dtype` (float32 for EMAGE_F16X3); W / bias / slope / a_scale / w_scale as for emage_gemm (bias and
 * slope are required); res: (nseq*L, ldr) `dtype` or NULL; out: (nseq*L, ldo) `dtype`.  Bit-identical to emage_gemm.
 *
 * emage_wav_block0 — WavEncoder block 0 in ONE launch (P:283-294 with Cin = 1): the slab is conv1 itself,
 *   y1 = leaky(conv(wav, w1) + b1, slope1), evaluated from the raw waveform into LDS (eval BatchNorm folded by the host,
 *   windows addressed as in emage_wav_conv_in); conv2 runs on it as above, and the epilogue adds the downsample shortcut
 *   conv(wav, wds) + bds of its own outputs before the activation.  out: (nwin*nclip*L, ldo), L = block-0 output length.
 *   Bit-identical to emage_wav_conv_in followed by emage_gemm; the (rows, 2C) first-layer tensor never reaches HBM.
 */
int emage_conv_slab(int dtype, const void* A, int lda, const void* W, const float* bias, const float* slope,
                    const void* res, int ldr, void* out, int ldo,
                    int nseq, int L, int C, int taps, int pad, float a_scale, float w_scale, void* stream);
int emage_wav_block0(int dtype, const float* wav, long ldw, int Lw, int nwin, long hop, int nclip,
                     const float* w1, const float* b1, float slope1, const float* wds, const float* bds,
                     int taps1, int stride1, int pad1,
                     const void* W2, const float* bias2, const float* slope2, int taps2, int pad2,
                     void* out, int ldo, int L, int C, float a_scale, float w_scale, void* stream);

/*
 * K4 — multi-head attention core, softmax(Q K^T / sqrt(hd)) V, no mask (nn.MultiheadAttention inside
 * the 15 decoder layers and 1 encoder layer, M:238-250,261).
 * q:  (B*Tq, ldq) `dtype`, head h at columns [h*hd, (h+1)*hd).
 * k:  (B*Tk, ldk) `dtype`, same head layout.
 * vt: V transposed, (B, vt_rows, ldvt) `dtype`: vt[(b*vt_rows + h*hd + d)*ldvt + t], vt_rows >= H*hd (several
 *     layers' V^T may share one buffer); ldvt % 32 == 0, ldvt >= Tk, columns [Tk, ldvt) must be finite (any finite value:
 *     their probabilities are exactly 0).  Nothing past the ldvt columns of a row is read: with Tk in 65..96 and ldvt = 96 the
 *     key slots [96, 128) of the 128-key path are zero operands, so what follows a V^T row in the buffer may be anything.
 * out:(B*Tq, ldo) `dtype`, head-concatenated like nn.MultiheadAttention before out_proj.
 * hd == 192 (768 / 4 heads, the only head size on this path), Tk <= 128.
 */
int emage_attention(int dtype, const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt, int vt_rows,
                    void* out, int ldo, int B, int H, int Tq, int Tk, int hd, void* stream);

/* emage_attention with the attention-probability dropout of a TRAINING forward (nn.MultiheadAttention in train mode,
 * torch's scaled_dot_product_attention math path): softmax(.) * pmask, then P V.  pmask: (B, H, Tq, Tk) fp32, the
 * factors bernoulli / (1 - p).  dtype EMAGE_F32 or EMAGE_F16X3. */
int emage_attention_dropout(int dtype, const void* q, int ldq, const void* k, int ldk, const void* vt, int ldvt, int vt_rows,
                            void* out, int ldo, int B, int H, int Tq, int Tk, int hd, const float* pmask, void* stream);

/*
 * One self-attention site in ONE launch: the qkv projection of emage_gemm (EMAGE_H2) and emage_attention on its q / k / V^T, with
 * q, k and v kept on chip.  One workgroup per (clip, head) computes the 64 x 576 block [q_h | k_h | v_h] of the projection, stages it in
 * LDS and runs the attention of that head.  `out` is bit for bit what the two-launch sequence writes:
 *     emage_gemm(dtype, A, lda, W, bias, out_f32 = qk (B T, 2 d), out_t = vt (V^T, t_col0 = 2 d, t_rows = T), M = B T, N = 3 d, Cp = d,
 *                a_scale, w_scale)   (with the LayerNorm fold: the same problem with ln_stats / ln_c / ln_eps, emage_gemm_grouped)
 *     emage_attention(dtype, qk, 2 d, qk + d, 2 d, vt, T, d, out, ldo, B, H, T, T, d / H)
 * Only T = 64, d = 768, H = 4 (hd = 192) and dtype EMAGE_H2 (with any activation shift: `out` is the image of that scale, A is read with
 * a_scale) are supported; anything else is EMAGE_EINVAL.
 * A:    (B T, lda) EMAGE_H2 image, lda % 8 == 0, lda >= d; with ln_stats the RAW pre-norm sum of a folded LayerNorm (emage_gemm_problem).
 * W:    (3 d, d) packed image of the in_proj weight times w_scale (rows q | k | v, as emage_gemm takes it); bias (3 d) fp32, required.
 * ln_stats / ln_c / ln_eps: the LayerNorm fold of emage_gemm_problem (ln_np = 24); NULL ln_stats = off, ln_c then required.
 * out:  (B T, ldo) EMAGE_H2 image, ldo % 8 == 0, ldo >= d.  Pointers 16-byte aligned.
 * The grouped form runs 1..4 independent problems of the same T / d / H in one launch (the part-wise decoder stacks in lock step).
 */
typedef struct emage_qkv_attention_problem {
    const void* A; const void* W; const float* bias; const float* ln_stats; const float* ln_c; void* out;
    int lda, ldo, B;
    float a_scale, w_scale, ln_eps;
} emage_qkv_attention_problem;
int emage_qkv_attention(int dtype, const void* A, int lda, const void* W, const float* bias, const float* ln_stats, const float* ln_c,
                        float ln_eps, void* out, int ldo, int B, int T, int d, int H, float a_scale, float w_scale, void* stream);
int emage_qkv_attention_grouped(int dtype, const emage_qkv_attention_problem* problems, int n_problems, int T, int d, int H, void* stream);

/*
 * One cross-attention site in ONE launch: the q projection of emage_gemm (EMAGE_H2) and emage_attention on it, with q kept on chip.  One
 * workgroup per (clip, head) computes the 64 x 192 block q_h of the projection, stages it with the layer's memory K_h / V_h^T in LDS and runs
 * the attention of that head.  `out` is bit for bit what the two-launch sequence writes:
 *     emage_gemm(dtype, A, lda, W, bias, out_f32 = q (B T, d), M = B T, N = d, Cp = d, a_scale, w_scale)
 *                (with the LayerNorm fold: the same problem with ln_stats / ln_c / ln_eps, emage_gemm_grouped)
 *     emage_attention(dtype, q, d, k, ldk, vt, ldvt, vt_rows, out, ldo, B, H, T, Tk, d / H)
 * (bit for bit as long as that emage_gemm takes its 64 x 64 tile, which it does below ~26 000 rows on 256 CUs: wider tiles merge the folded
 * LayerNorm's partial statistics in another order).
 * Only T = Tk = 64, d = 768, H = 4 (hd = 192) and dtype EMAGE_H2 (with any activation shift) are supported; anything else is EMAGE_EINVAL.
 * A, W, bias, ln_stats / ln_c / ln_eps, out: as for emage_qkv_attention, W the (d, d) packed q projection.
 * k:    (B Tk, ldk) float32, head h at columns [h hd, (h + 1) hd); ldk % 4 == 0, ldk >= d (a column block of several layers' keys is a view).
 * vt:   V transposed, (B, vt_rows, ldvt) float32 as emage_attention takes it: vt_rows >= d, ldvt % 32 == 0, ldvt >= 64.
 * Pointers 16-byte aligned; every operand spans less than 2 GiB.
 * The grouped form runs 1..4 independent problems in one launch (the part-wise decoder stacks in lock step).
 */
typedef struct emage_q_attention_problem {
    const void* A; const void* W; const float* bias; const float* ln_stats; const float* ln_c;
    const float* k; const float* vt; void* out;
    int lda, ldk, ldvt, vt_rows, ldo, B;
    float a_scale, w_scale, ln_eps;
} emage_q_attention_problem;
int emage_q_attention(int dtype, const emage_q_attention_problem* problem, int T, int Tk, int d, int H, void* stream);
int emage_q_attention_grouped(int dtype, const emage_q_attention_problem* problems, int n_problems, int T, int Tk, int d, int H, void* stream);

/*
 * The same site when the layer's memory K / V^T are a Linear projection of a feature image that nothing else reads (the two decoder stacks:
 * their memory projection composed with the K / V projections at packing time, K = (a Wp^T + bp) Wk^T + bk = a (Wk Wp)^T + (Wk bp + bk)): the
 * workgroup of (clip, head) computes K_h / V_h of its 64 memory frames itself, then q_h, then the attention.  `out` is bit for bit
 *     emage_gemm(dtype, mem, ldm, Wkv, bias_kv, out_f32 = K (B Tk, kv_layers d), out_t = V^T (B, kv_layers d, 64), t_col0 = kv_layers d, t_rows = 64,
 *                M = B Tk, N = 2 kv_layers d, Cp = km, a_scale, wkv_scale)
 *     emage_q_attention(... k = K + kv_layer d, ldk = kv_layers d, vt = V^T + kv_layer d 64, vt_rows = kv_layers d ...)
 * A, W, bias, ln_stats / ln_c / ln_eps, out, lda, ldo, B, a_scale, w_scale: as for emage_q_attention.
 * mem:  (B Tk, ldm) EMAGE_H2 image of the memory features, km columns used; ldm % 8 == 0, ldm >= km; km % 32 == 0, 32 <= km <= d.
 * Wkv:  (2 kv_layers d, km) packed image times wkv_scale, rows [K_0 .. K_n | V_0 .. V_n] (d rows per layer); bias_kv (2 kv_layers d) fp32.
 * kv_layer: the layer of the stack this site belongs to, 0 <= kv_layer < kv_layers <= 64.
 * Only T = Tk = 64, d = 768, H = 4 and dtype EMAGE_H2 (with any activation shift); anything else is EMAGE_EINVAL.  Pointers 16-byte aligned.
 * The grouped form runs 1..4 independent problems in one launch (the two stacks in lock step).
 */
typedef struct emage_qm_attention_problem {
    const void* A; const void* W; const float* bias; const float* ln_stats; const float* ln_c;
    const void* mem; const void* Wkv; const float* bias_kv; void* out;
    int lda, ldm, km, kv_layers, kv_layer, ldo, B;
    float a_scale, w_scale, wkv_scale, ln_eps;
} emage_qm_attention_problem;
int emage_qm_attention(int dtype, const emage_qm_attention_problem* problem, int T, int Tk, int d, int H, void* stream);
int emage_qm_attention_grouped(int dtype, const emage_qm_attention_problem* problems, int n_problems, int T, int Tk, int d, int H, void* stream);

/*
 * K5 — LayerNorm(C, eps) over rows (post-norm of every transformer sub-layer):
 *   y = (x - mean) * rsqrt(var + eps) * gamma + beta (+ add[m][:])
 * x: (M, ldx) `dtype` — the residual stream is stored in the compute dtype (fp32 in parity mode, bf16 in bf16
 * mode); statistics and the affine map are fp32.  add: (M, ldadd) `dtype` or NULL (folds the positional /
 * speaker / skip adds that follow a LayerNorm, M:304-305,312).  y_f32: (M, ldy) fp32 or NULL;
 * y: (M, ldy) `dtype` or NULL.  C % 64 == 0, C <= 1024.
 */
int emage_layernorm(int dtype, const void* x, int ldx, const float* gamma, const float* beta, float eps,
                    const void* add, int ldadd, float* y_f32, void* y, int ldy, int M, int C, void* stream);

/*
 * K11 — elementwise glue.
 * emage_add: out[m] = a[m] + b[m % mod_b] (+ c[m % mod_c]); operand k (a=0,b=1,c=2) is fp32 when bit k of
 *   f32_mask is set, else `dtype` (mod_* = 0: no wrap; mod = T broadcasts a (T,C) positional table over the
 *   batch, P:341-343); writes fp32 and/or `dtype`.  C % 4 == 0.
 * emage_pack_motion: one window of the masked-motion input -> `dtype`, (B*T, ldo), columns [C, n_store) zero:
 *   where(mask == 1, mask_embedding, motion) (M:267-268); with `seed` != NULL the first `pre` frames are
 *   where(mask == 0, motion, seed) and count as unmasked — the seed splice of inference() (M:386-391).  motion / mask:
 *   fp32, frame (b, t) at b*ldb + t*C (a window of a longer (B, L, C) tensor is read in place); seed: frame (b, t) at
 *   b*ld_seed + t*C.
 * emage_pack_motion_hints: emage_pack_motion with a table-driven source (recordings.RecordingRunner(hints=True): keyframes, kept body
 *   parts).  The hint store is two arrays of store_rows rows with one pitch ld >= C: motion (fp32) and keep (uint8, the reference's mask
 *   values — 1: generate this element, 0: this element is given; only 0 and 1 occur).  table: B rows of two 64-bit words on the device,
 *   {store row of this window's frame 0, avail}: frame t of batch row b reads store row table[b][0] + t when t < avail; frames
 *   t >= avail read nothing and behave as keep = 1 (avail = 0: a row without hints).  Per element n < C, as emage_pack_motion:
 *   seed != NULL and t < pre: keep == 0 ? motion : seed[b, t, n]; otherwise keep == 1 ? mask_embedding[n] : motion.  Every dtype of
 *   emage_pack_motion, the EMAGE_H2 codes with their activation-shift bits included.  With ld % 8 == 0 (ld = 344 for C = 337), motion
 *   16-byte and keep 8-byte aligned, the EMAGE_H2 form reads a group of 8 columns as two 16-byte loads and one 8-byte flag word; any other
 *   ld >= C reads element by element.  A table row with avail < 0, avail > T, first < 0 or first + avail > store_rows is treated as
 *   avail = 0 and ORs 4 into *status (the sticky int32 word of emage_gather_windows / emage_copy_segments); nothing outside the two
 *   arrays is ever read.
 * emage_cast_pad: fp32 (M,C) -> `dtype` (M, ldo) with zero tail [C, n_store).
 */
int emage_add(int dtype, const void* a, int lda, const void* b, int ldb, int mod_b, const void* c, int ldc, int mod_c,
              int f32_mask, float* out_f32, void* out, int ldo, int M, int C, void* stream);
int emage_pack_motion(int dtype, const float* motion, const float* mask, long ldb, const float* mask_embedding,
                      const float* seed, long ld_seed, int pre,
                      void* out, int ldo, int n_store, int B, int T, int C, void* stream);
int emage_pack_motion_hints(int dtype, const float* motion, const unsigned char* keep, long store_rows, int ld, const long long* table,
                            const float* mask_embedding, const float* seed, long ld_seed, int pre,
                            void* out, int ldo, int n_store, int B, int T, int C, int* status, void* stream);
int emage_cast_pad(int dtype, const float* src, int lds, void* out, int ldo, int n_store, int M, int C, void* stream);

/*
 * K9 — rotation conversions (P:16-104), elementwise over n joints.
 */
int emage_rot6d_to_axis_angle(const float* rot6d, float* aa, int n, void* stream);
int emage_axis_angle_to_rot6d(const float* aa, float* rot6d, int n, void* stream);

/*
 * K9+K11 — EmageVQModel.decode's merge (M:137-188) in one pass and without host syncs:
 * part decoder outputs -> rot6d->axis-angle per part joint, scatter into the 55 SMPL-X joints
 * (recover_from_mask_ts, P:118-132; jaw at joint 22), re-encode to rot6d, append trans/contact.
 * face: (M, ldface) fp32 [6 jaw rot6d | 100 expression] or NULL (zeros); upper: (M, ldup) 78;
 * hands: (M, ldh) 180; lower: (M, ldlow) [54 rot6d | 3 trans-vel | 4 contact] or NULL.
 * Outputs (any may be NULL): axis_angle (M,165), motion (M,337) = [330 rot6d | 7], expression (M,100).
 */
int emage_merge_parts(const float* face, int ldface, const float* upper, int ldup, const float* hands, int ldh,
                      const float* lower, int ldlow, float* axis_angle, float* motion, float* expression,
                      int M, void* stream);

/*
 * K10 — velocity2position (P:107-115) for get_global_motion (M:195-205):
 *   trans[b][0][x|z] = init[b][x|z]; trans[b][t][x|z] = vel[b][t-1][x|z]*dt + trans[b][t-1][x|z]
 *   trans[b][t][y] = vel[b][t][y]        (sequential fp32, product rounded before the add)
 * vel: (B*T, ldv) fp32, the 3 velocity channels start at column col0; init: fp32, clip b at init + b*ld_init
 * (ld_init = 0 broadcasts one start position, M:198-200).
 */
int emage_velocity_to_position(const float* vel, int ldv, int col0, const float* init, int ld_init, float dt,
                               float* trans, int B, int T, void* stream);

/*
 * ---- DisCo / CaMN: models/disco_audio/modeling_disco_audio.py (D:), models/camn_audio/
 * modeling_camn_audio.py (C:).  Their WavEncoder, MLPs and the LSTM input projections run on emage_wav_conv_in /
 * emage_gemm; the entry points below are what is specific to them.  float32 tensors throughout.
 *
 * emage_lstm_step — one time step of ONE direction of nn.LSTM (D:190-195,252; C:204-218,261-268) for the whole batch:
 *   gates = gates_x[b] + h_prev[b] W_hh^T;  c' = sigmoid(f) c + sigmoid(i) tanh(g);  h' = sigmoid(o) tanh(c')
 * with the gate rows INTERLEAVED per hidden unit: column 4u + g of `gates` (g = input, forget, cell, output — torch's
 * packed order regrouped by the host), so one lane owns all four gates of a unit.  h_prev: (B, ld_hprev) the previous
 * step's hidden state (zeros for the first step); w_hh: (4H, H) in `dtype` (EMAGE_F32, or EMAGE_F16X3 = the host-split
 * image of emage_gemm with w_scale / a_scale); gates_x: (B, ld_gx) this step's rows of the input projection
 * x_t W_ih^T + b_ih + b_hh (same interleaved layout); cstate: (B, ldc) updated in place; h_out: (B, ld_hout).
 * Rows may be strided views (step t of a (B, T, .) tensor: ld = T * width).  H % 64 == 0.
 */
int emage_lstm_step(int dtype, const float* h_prev, int ld_hprev, const void* w_hh, float w_scale, float a_scale,
                    const float* gates_x, int ld_gx, float* cstate, int ldc, float* h_out, int ld_hout,
                    int B, int H, void* stream);

/* Both directions of one layer in one launch: problem 0 = forward direction at its time step, problem 1 = backward direction at its
 * own; arguments as for emage_lstm_step, per direction where they differ (gate rows / cell states / outputs share their row strides). */
int emage_lstm_step_pair(int dtype, const float* h_prev0, const float* h_prev1, int ld_hprev0, int ld_hprev1,
                         const void* w_hh0, const void* w_hh1, float w_scale0, float w_scale1, float a_scale,
                         const float* gates_x0, const float* gates_x1, int ld_gx,
                         float* cstate0, float* cstate1, int ldc, float* h_out0, float* h_out1, int ld_hout,
                         int B, int H, void* stream);

/*
 * emage_lstm_layer — the whole recurrence of one bidirectional nn.LSTM layer in ONE launch per <= n_CU / (2 * H/16) * 64 clips
 * (D:190-195,252; C:204-218,261-268): persistent blocks keep their W_hh slice (both split-fp16 planes) and their cell state in
 * registers for all T steps and exchange h_t through the layer output as write-through stores the consumers poll (the data is the flag;
 * csrc/lstmseq.hip).  A block owns 64 clips — or 32 when the whole batch then still fits one launch (B <= n_CU / (2 * H/16) * 32), so that
 * every CU has a block; the result does not depend on that choice.
 * Bit-identical to T emage_lstm_step_pair launches with zero initial state.  dtype: EMAGE_F16X3 only; H = 256 or 512.
 *   gates_x  (B, T, >= 8H) fp32: the input projection of every step incl. both biases, columns dir * 4H + 4u + g
 *            (row strides ld_gx_b per clip, ld_gx_t per step, in floats)
 *   w_hh0/1  the directions' recurrent weights packed like emage_gemm's F16X3 W operand (rows 4u + g), scales w_scale0/1
 *   hseq     (B, T, >= 2H) fp32 out: h_t of the forward direction in columns [0, H), of the backward one in [H, 2H)
 *   sync     scratch of emage_lstm_layer_sync_words(B, H) 32-bit words (zeroed by the call, on the stream).  After the
 *            stream has been synchronised, word EMAGE_LSTM_SYNC_ERROR_WORD of each EMAGE_LSTM_SYNC_WORDS_PER_LAUNCH-word
 *            record is non-zero if a block gave up waiting for its group (~1 s: blocks not co-resident) — the output
 *            is then invalid; the Python layer raises.
 */
#define EMAGE_LSTM_SYNC_WORDS_PER_LAUNCH 544
#define EMAGE_LSTM_SYNC_ERROR_WORD 512
int emage_lstm_layer_sync_words(int B, int H);
/* returns EMAGE_EINVAL (<= 0 words) when the CURRENT device cannot host the recurrence (fewer than 2 * H/16 co-resident blocks:
 * a compute partition / CU-masked queue): callers then take emage_lstm_step_pair, which produces the same bits.
 * emage_lstm_layer_health: counter[0] += number of launch records of `sync` whose error word is set; meant to run on the same
 * stream behind the emage_lstm_layer launches (inside a captured graph), so one device counter carries "a block was lost". */
int emage_lstm_layer_health(const unsigned* sync, int sync_words, int* counter, void* stream);
int emage_lstm_layer(int dtype, const float* gates_x, long ld_gx_b, int ld_gx_t, const void* w_hh0, const void* w_hh1,
                     float w_scale0, float w_scale1, float a_scale, float* hseq, long ld_h_b, int ld_h_t,
                     int B, int T, int H, unsigned* sync, int sync_words, void* stream);
/* emage_lstm_layer_lengths: the same launch for clips of DIFFERENT lengths (recordings generated as one batch).  lengths: device array of
 * B ints, or NULL (= emage_lstm_layer, which forwards here).  Clip b is a sequence of len_b = clamp(lengths[b], 0, T) steps: at every
 * t >= len_b both directions' cell state and h_t are exactly 0.0f for that clip (selected, never multiplied: gates_x there may hold
 * anything, NaN included), so the backward direction reaches t = len_b - 1 with zero state and hseq[b][0 .. len_b) carries the BITS of
 * that clip run alone with T = len_b; hseq[b][len_b .. T) is 0.  The hand-over protocol is untouched (masked steps still store every word
 * of h_t), so the cost stays that of T steps: lengths shorten no launch. */
int emage_lstm_layer_lengths(int dtype, const float* gates_x, long ld_gx_b, int ld_gx_t, const void* w_hh0, const void* w_hh1,
                             float w_scale0, float w_scale1, float a_scale, float* hseq, long ld_h_b, int ld_h_t,
                             int B, int T, int H, const int* lengths, unsigned* sync, int sync_words, void* stream);

/* DisCo's content blend (D:244-247): out = softmax(sel[:, 0:2])[0] * c1 + softmax(...)[1] * c2, rows of C channels. */
int emage_softmax2_mix(const float* sel, int ld_sel, const float* c1, int ld1, const float* c2, int ld2,
                       float* out, int ldo, int M, int C, void* stream);

/*
 * The [speaker | seed motion | is-seed | zero pad] tail of the LSTM input rows (D:200-243, C:224-259): row (b, t) gets
 * speaker_table[speaker_id[b]] (speaker_f values), then the reference's padded seed tensor at frame src_map[t]
 * (frames < seed_frames carry seed_motion[b][frame] (pose_dims values, or zeros when seed_motion is NULL) and flag 1;
 * src_map[t] < 0 or >= seed_frames: zeros), then zeros up to n_store.  src_map: T ints on the device.
 */
int emage_lstm_inputs(const float* speaker_table, const int64_t* speaker_id, int speaker_f,
                      const float* seed_motion, long ld_seed_b, int pose_dims, int seed_frames, const int* src_map,
                      float* out, int ldo, int n_store, int B, int T, void* stream);

/*
 * rot-6D -> axis-angle scattered into the SMPL-X joint order (D:256-258 + recover_from_mask_ts D:81-96):
 * joint j takes the conversion of rot6d[m][6*slot .. 6*slot+5] with slot = slot_of_joint[j], or zeros when slot < 0.
 * rot6d: (M, ld) fp32; slot_of_joint: n_joints ints on the device; axis_angle: (M, n_joints*3).
 */
int emage_rot6d_scatter(const float* rot6d, int ld, const int* slot_of_joint, float* axis_angle, int M, int n_joints, void* stream);

/* counter[0] += number of non-finite values in the contiguous fp32 array x[0 .. n): the runners' end-of-batch health check. */
int emage_count_nonfinite(const float* x, long n, int* counter, void* stream);
/* The same over `count` <= 16 tensors in ONE launch (contiguous fp32, ns[i] elements each; the pointer table is read on the host at call time
 * and travels by value): the end-of-batch health check of the clip runners. */
int emage_count_nonfinite_multi(const float* const* xs, const long* ns, int count, int* counter, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Train-mode forward (train_emage_audio.py:130-204): what differs from the inference path.
 * ------------------------------------------------------------------------------------------------------------------ */

/*
 * nn.BatchNorm1d in training mode, statistics: per-channel batch mean and BIASED variance over the M rows (all clips x all
 * positions) of a channels-last fp32 tensor x (M, ldx), float64 accumulation; running_mean / running_var (either may be
 * NULL) are updated in place as torch does: r = (1 - momentum) * r + momentum * {mean, UNBIASED variance}
 * (processing_emage_audio.py:262-294 with nn.BatchNorm1d semantics; nn.SyncBatchNorm at world size 1).
 * workspace: emage_bn_stats_workspace_bytes(M, C) bytes, 8-byte aligned.
 */
long emage_bn_stats_workspace_bytes(int M, int C);
int emage_bn_stats(const float* x, int ldx, int M, int C, void* workspace, long workspace_bytes,
                   float* mean, float* var, float* running_mean, float* running_var, float momentum, void* stream);

/*
 * The normalisation with what follows it in BasicBlock.forward (P:283-294):
 *   out = LeakyReLU((x - mean) / sqrt(var + eps) * gamma + beta + shortcut, slope)
 * shortcut: none (sc NULL) | sc raw (sc_mean NULL) | sc batch-normalised with its own statistics (the downsample branch).
 */
int emage_bn_apply(const float* x, int ldx, const float* mean, const float* var, const float* gamma, const float* beta,
                   const float* sc, int ld_sc, const float* sc_mean, const float* sc_var, const float* sc_gamma, const float* sc_beta,
                   float eps, float slope, float* out, int ldo, int M, int C, void* stream);

/*
 * out = a * mask (+ b): nn.Dropout with a given mask and the residual add that follows it in nn.Transformer*Layer.
 * mask_t_rows = T > 0: the mask is stored (T, M / T, C) — the (T, B, d) layout the reference's layers see — while the
 * rows of a / b / out run (B, T); 0: same row order.
 */
int emage_mul_add(const float* a, int lda, const float* mask, int ld_mask, int mask_t_rows, const float* b, int ldb,
                  float* out, int ldo, int M, int C, void* stream);

/*
 * The losses of train_emage_audio.py:106-130, accumulated into a float64 device scalar: loss[0] += weight * value.
 *   emage_mse_loss: value = mean((pred - target)^2) over the (M, C) fp32 views           (F.mse_loss, T:108-111)
 *   emage_nll_loss: value = mean over rows of -log_softmax(logits[m])[index[m]]           (NLLLoss(log_softmax), T:113-128)
 * workspace: EMAGE_LOSS_WORKSPACE_BYTES bytes, 8-byte aligned, zeroed once by the caller.  An index outside [0, K) contributes
 * nothing and sets the last 8-byte slot of the workspace non-zero (sticky; torch raises there; the Python layer checks it).
 */
#define EMAGE_LOSS_WORKSPACE_BYTES 8192
int emage_mse_loss(const float* pred, int ld_pred, const float* target, int ld_target, int M, int C, float weight,
                   double* loss, void* workspace, void* stream);
int emage_nll_loss(const float* logits, int ld, const int64_t* index, int M, int K, float weight, double* loss, void* workspace, void* stream);

/* ------------------------------------------------------------------------------------------------------------------
 * Backward building blocks of the training step (first functional versions: fp32 VALU code with float64 reductions; the
 * contractions of the Linear layers — dX = dY W, dW = dY^T X — are emage_gemm launches on transposed operands).
 * ------------------------------------------------------------------------------------------------------------------ */

/* out (N, ld_out) = in (M, ld_in) transposed, fp32. */
int emage_transpose_f32(const float* in, int ld_in, float* out, int ld_out, int M, int N, void* stream);

/* out[c] (+)= sum_m x[m][c] (* y[m][c] when y is given): bias / LayerNorm-affine gradients.  float64 block partials added in
 * block order (deterministic); workspace: emage_col_sum_chunks(M) * C * 8 bytes.  out == NULL (round 5): only the partials are
 * written (partial[chunk * C + c]); a later emage_col_sum_finalize_multi ends this reduction together with others.
 *
 * emage_col_sum_finalize_multi — the finalize step of up to 64 chunked column reductions in ONE launch (a training step ends ~600 of
 * them: bias gradients from emage_grad_prep, LayerNorm / embedding gradients from emage_col_sum).  `entries`: HOST memory, read during
 * the call (the table travels by value in the kernel argument segment: nothing to allocate, and a captured launch keeps its own copy).
 * Entry by entry the arithmetic (and the bits) of the finalize launch inside emage_col_sum / emage_grad_prep.  No two entries of one
 * call may name overlapping `out` ranges. */
typedef struct emage_finalize_entry {
    const double* partial;      /* chunks x C float64 partials: partial[chunk * C + c] */
    float* out;                 /* C floats */
    int chunks, C, accumulate;  /* accumulate != 0: out[c] += sum, else out[c] = sum */
} emage_finalize_entry;
int emage_col_sum_chunks(int M);
int emage_col_sum_finalize_multi(const emage_finalize_entry* entries, int n_entries, void* stream);
int emage_col_sum(const float* x, int ldx, const float* y, int ldy, int M, int C, float* out, int accumulate,
                  void* workspace, long workspace_bytes, void* stream);

/* out = dy * (y > 0 ? 1 : slope): LeakyReLU / ReLU backward from the saved OUTPUT y of the activation. */
int emage_act_backward(const float* dy, int ld_dy, const float* y, int ld_y, float slope, float* out, int ldo, int M, int C, void* stream);

/* The gradient operands of one nn.Linear's backward (what loss.backward() computes per layer, train_emage_audio.py:174) from the gradient dy
 * (M, C) of its output in ONE pass: dpre = dy * (y > 0 ? 1 : slope) when the layer's saved output y is given (else dpre = dy);
 *   out_h (M, n_store >= C, % 8): EMAGE_H2 image of scale * dpre, zero tail columns            (operand of dX = dpre W)
 *   out_t (C, m_store >= M, % 8): EMAGE_H2 image of scale * dpre^T, zero tail columns          (operand of dW = dpre^T X)
 *   bias_grad[c] (+)= sum_m dpre[m][c] (float64 partials per 64 rows in `workspace`, >= ceil(M / 64) * C * 8 bytes, added in row order)
 * any of the three outputs may be NULL; scale a power of two (the loss scale of the split-fp16 backward).  `workspace` without
 * bias_grad (round 5): the ceil(M / 64) x C partials are written and left for emage_col_sum_finalize_multi. */
int emage_grad_prep(const float* dy, int ld_dy, const float* y, int ld_y, float slope, int M, int C, float scale,
                    void* out_h, int ldh, int n_store, void* out_t, int ldt, int m_store,
                    float* bias_grad, int accumulate, void* workspace, long workspace_bytes, void* stream);

/* nn.LayerNorm backward for input rows x (M, C): dx, and dy_xhat = dy * (x - mean) * rstd (column sums of dy_xhat / dy are
 * the weight / bias gradients: emage_col_sum). */
int emage_layernorm_backward(const float* x, int ldx, const float* gamma, const float* dy, int ld_dy, float eps,
                             float* dx, int ld_dx, float* dy_xhat, int ld_t, int M, int C, void* stream);

/* nn.LayerNorm backward with its affine gradients in two launches: dx as emage_layernorm_backward (the same bits), and
 * dgamma[c] (+)= sum_m dy[m][c] * xhat[m][c], dbeta[c] (+)= sum_m dy[m][c] (float64 partials per `rows_per_block` rows — 4 or 16 — in
 * `workspace`, added in row order; `accumulate`: into the parameters' gradient accumulators, loss.backward()'s accumulation over the three
 * forwards of a step, T:174).  C <= 1024. */
long emage_layernorm_backward_affine_workspace_bytes(int M, int C, int rows_per_block);
int emage_layernorm_backward_affine(const float* x, int ldx, const float* gamma, const float* dy, int ld_dy, float eps, float* dx, int ld_dx,
                                    float* dgamma, float* dbeta, int accumulate, int M, int C, int rows_per_block,
                                    void* workspace, long workspace_bytes, void* stream);

/* Backward of emage_attention / emage_attention_dropout (same operand layouts; pmask may be NULL): dq (B*Tq, .), dk, dv (B*Tk, .)
 * in row layout with head h at columns [h*hd, (h+1)*hd).  The probabilities are recomputed. */
int emage_attention_backward(const float* q, int ldq, const float* k, int ldk, const float* vt, int ldvt, int vt_rows, const float* pmask,
                             const float* d_out, int ld_do, float* dq, int ld_dq, float* dk, int ld_dk, float* dv, int ld_dv,
                             int B, int H, int Tq, int Tk, int hd, void* stream);

/* Gradients of the two losses w.r.t. their predictions: grad = weight * 2 (pred - target) / (M C);
 * grad = weight * (softmax(logits) - onehot(index)) / M. */
int emage_mse_loss_grad(const float* pred, int ld_pred, const float* target, int ld_target, int M, int C, float weight,
                        float* grad, int ld_grad, void* stream);
int emage_nll_loss_grad(const float* logits, int ld, const int64_t* index, int M, int K, float weight, float* grad, int ld_grad, void* stream);

/*
 * Conv1d backward through emage_gemm: dW (N, taps*C) = dY^T (N, M) x im2col(X)^T, dX = col2im(dY W).
 *   emage_im2col_t: out[(tap*C + c)][m] = X[seq*Lin + l*stride - pad + tap][c] (0 outside the sequence), m = seq*Lout + l,
 *                   out is (taps*C, ld_out >= nseq*Lout) fp32 with the tail columns left untouched (pre-zeroed by the caller)
 *   emage_col2im:   dx[seq*Lin + r][c] = sum of dcol[seq*Lout + l][tap*C + c] over the (l, tap) that read input position r
 */
int emage_im2col_t(const float* x, int ldx, int C, int taps, int stride, int pad, int Lin, int Lout, int nseq,
                   float* out, long ld_out, void* stream);
/* emage_im2col_t with the result as an EMAGE_H2 image (taps * C, ld_out): columns [nseq * Lout, rup64(nseq * Lout)) are written as zeros. */
int emage_im2col_t_h2(const float* x, int ldx, int C, int taps, int stride, int pad, int Lin, int Lout, int nseq,
                      void* out, long ld_out, void* stream);
int emage_col2im(const float* dcol, long ld, int C, int taps, int stride, int pad, int Lin, int Lout, int nseq, float* dx, int ldx, void* stream);

/* nn.BatchNorm1d (training) backward on channels-last rows: dgamma = sum dy * xhat, dbeta = sum dy (float64 sums),
 * dx = gamma * rstd * (dy - dbeta / M - xhat * dgamma / M).  workspace as for emage_bn_stats. */
int emage_bn_backward(const float* x, int ldx, const float* mean, const float* var, const float* gamma, float eps, const float* dy, int ld_dy,
                      float* dx, int ld_dx, float* dgamma, float* dbeta, int M, int C, void* workspace, long workspace_bytes, void* stream);

/* The two halves of emage_bn_backward on their own: nn.SyncBatchNorm all-reduces the per-channel sums between them
 * (train_emage_audio.py:248); `count` is the GLOBAL number of rows behind mean / var. */
int emage_bn_backward_sums(const float* x, int ldx, const float* mean, const float* var, float eps, const float* dy, int ld_dy,
                           float* sum_dy_xhat, float* sum_dy, int M, int C, void* workspace, long workspace_bytes, void* stream);
int emage_bn_backward_apply(const float* x, int ldx, const float* mean, const float* var, const float* gamma, float eps, const float* dy, int ld_dy,
                            const float* sum_dy_xhat, const float* sum_dy, long count, float* dx, int ld_dx, int M, int C, void* stream);

/* Weight gradient of emage_wav_conv_in (Cin = 1): dw[c][tap] = sum_m dy[m][c] * wav[seq][l*stride - pad + tap]. */
long emage_wav_conv_in_backward_workspace_bytes(int M, int C, int taps);
int emage_wav_conv_in_backward(const float* dy, int ld_dy, const float* wav, long ldw, int L, int B, int Lout, int C, int taps, int stride, int pad,
                               float* dw, void* workspace, long workspace_bytes, void* stream);

/* torch.optim.Adam (no amsgrad) on one flat fp32 tensor of n elements, in place (train_emage_audio.py:258-265): step is the
 * 1-based step count of this parameter. */
int emage_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, int step,
                    float lr, float beta1, float beta2, float eps, float weight_decay, void* stream);

/* fp32 (M, C) rows -> EMAGE_H2 image of src * scale (scale a power of two: gradients are pre-scaled so that their fp16 planes stay
 * normal).  transpose = 0: out (M, n_store), zero tail [C, n_store);  transpose != 0: out (C, n_store) with out[c][m] = src[m][c] * scale
 * and a zero tail [M, n_store) — the operands of the backward contractions of a training step (dW = dY^T X contracts over the rows). */
int emage_h2_cast(const float* src, int lds, void* out, int ldo, int n_store, int M, int C, float scale, int transpose, void* stream);

/* fp32 (N, K) weight rows (K % 32 == 0, 16-byte aligned rows) -> the EMAGE_F16X3 weight operand of w * scale (scale a power of two), the image
 * emage_gemm takes as `w` in that mode: per row and 32-k K-tile 128 bytes = [16 x 4 fp16 hi | 16 x 4 fp16 lo], 16-byte chunk g of a plane holding
 * k = 4g..4g+3, 16+4g..16+4g+3.  out: (N, ldo) 4-byte elements, ldo >= K.  A training step re-packs every weight behind each Adam update
 * (train_emage_audio.py:174-176 changes them): one launch per operand instead of the host-side tensor arithmetic. */
int emage_f16x3_pack_weights(const float* w, int ldw, void* out, int ldo, int N, int K, float scale, void* stream);

/* Multi-tensor Adam: ONE launch over every parameter.  table: per tensor five 64-bit words {param, grad, exp_avg, exp_avg_sq, n} (device
 * pointers / element count); block b updates elements [block_chunk[b] * C, +C) of tensor block_tensor[b], C = emage_adam_multi_chunk().
 * step_dev (one int32 on the device) overrides `step` when non-NULL (captured graphs).  grad_scale multiplies every gradient first (the
 * 1 / world_size of the data-parallel average); zero_grad != 0 clears the gradient behind the update.  Arithmetic of emage_adam_step.
 * skip (one int32 on the device, may be NULL): when non-zero at launch time — the trainer's count of non-finite gradient words
 * (emage_count_nonfinite over the gradient buckets, inside the same captured step) — parameters and moments are left untouched (the
 * gradients are still cleared): an overflow of the split-fp16 backward never reaches the weights (the step-skip of loss-scaled training). */
int emage_adam_multi_chunk(void);
int emage_adam_multi(const long long* table, const int* block_tensor, const int* block_chunk, int n_blocks, const int* step_dev, int step,
                     float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale, int zero_grad, const int* skip,
                     void* stream);

/* emage_adam_multi with one more gradient factor read from DEVICE memory: grad_scale_dev (one fp32, may be NULL).  Every block forms
 * s = grad_scale * *grad_scale_dev once, in fp32, and uses g[i] * s — the clip coefficient of emage_grad_sumsq_multi reaches Adam without a
 * pass over the gradients and without the host.  NULL is emage_adam_multi itself (the same kernel; emage_adam_multi passes NULL). */
int emage_adam_multi_scaled(const long long* table, const int* block_tensor, const int* block_chunk, int n_blocks, const int* step_dev, int step,
                            float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale, const float* grad_scale_dev,
                            int zero_grad, const int* skip, void* stream);

/* Global gradient norm and clip coefficient (torch.nn.utils.clip_grad_norm_, norm_type 2; train_emage_audio.py:179-180 with
 * configs/emage_audio.yaml:67 max_grad_norm) over the gradients of an emage_adam_multi table (word 1 of a tensor's five is its gradient, word 4
 * its n; block_tensor / block_chunk / n_blocks as there, the blocks of a tensor consecutive with ascending chunks; n_tensors rows).  In float64:
 *   tensor_sumsq[t] = sum of g^2 over tensor t (n_tensors doubles), total_sumsq = their sum (one double);
 * every g is squared as a double (exact), per-block partial sums go to `workspace` and a finalize launch adds each tensor's partials and then
 * the tensors in table order with a fixed tree: no atomics, the same input gives the same bits.  Two fp32 device scalars follow:
 *   norm = pre_scale * sqrt(total_sumsq)            (pre_scale: the 1 / world_size of a data-parallel SUM of gradients; 1 otherwise)
 *   coef = min(1, max_norm / (norm + 1e-6))         (evaluated in double from the unrounded norm, rounded to fp32 once)
 * max_norm <= 0 or +inf: coef = 1.0f exactly (the norm is still reported).  Non-finite gradients: norm is inf / NaN and coef what the formula
 * gives (0 or NaN), as in torch.  Gradients need 4-byte alignment only.  workspace: 8-byte aligned, emage_grad_norm_workspace_bytes(n_blocks,
 * n_tensors) bytes (0 for invalid counts), no initialisation needed.  Two launches. */
long emage_grad_norm_workspace_bytes(int n_blocks, int n_tensors);
int emage_grad_sumsq_multi(const long long* table, const int* block_tensor, const int* block_chunk, int n_blocks, int n_tensors,
                           double pre_scale, double max_norm, double* tensor_sumsq, double* total_sumsq, float* norm, float* coef,
                           void* workspace, long workspace_bytes, void* stream);

/* g[i] *= *coef (one fp32 on the device) over every gradient of an emage_adam_multi table, one launch: the second half of a stand-alone
 * clip_grad_norm_ (the trainers fold coef into Adam instead: emage_adam_multi_scaled). */
int emage_scale_multi(const long long* table, const int* block_tensor, const int* block_chunk, int n_blocks, const float* coef, void* stream);

/* nn.Dropout's keep mask drawn on the device (T:241-250 dropout = 0.1 in every transformer layer, P:331,343): out[i] = bernoulli(1 - p) / (1 - p)
 * from Philox4x32-10 with key = seed, counter = (i / 4, mask_id, step): a pure function of its arguments (no generator state; step_dev, one
 * int32 on the device, overrides `step` when non-NULL so a captured training step draws fresh masks on every replay).  The stream is this
 * library's own (csrc/train.hip), not torch's. */
int emage_dropout_mask(float* out, long n, float p, unsigned long long seed, unsigned mask_id, const int* step_dev, int step, void* stream);

/* emage_mul_add with the mask of emage_dropout_mask(seed, mask_id, step) drawn inside the kernel instead of read from memory: out = a * keep (+ b),
 * keep = element (mask row, c) of that (M, C) mask (mask_t_rows as in emage_mul_add), C % 4 == 0.  The same bits as the two calls; the forward
 * and the backward of a dropout site (F.dropout inside nn.Transformer*Layer, train_emage_audio.py:156-172) draw the mask from the key each. */
int emage_mul_add_philox(const float* a, int lda, float p, unsigned long long seed, unsigned mask_id, const int* step_dev, int step, int mask_t_rows,
                         const float* b, int ldb, float* out, int ldo, int M, int C, void* stream);

/* emage_adam_step with the 1-based step count read from device memory (`step`: one int32), for a step captured in a hipGraph. */
int emage_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, const int* step,
                        float lr, float beta1, float beta2, float eps, float weight_decay, void* stream);

/* A training batch cut out of a device-resident clip store in ONE launch (datasets/beat2.py:97-129 BEAT2DatasetEamgeFootContact.__getitem__ and the
 * DataLoader's collation, train_emage_audio.py:277), no host work per step.  The store: every recording's frames end to end in four flat fp32 arrays
 * poses (total_frames, 165), expressions (.., 100), trans (.., 3), contact (.., 4) and its audio end to end in one array of total_samples samples,
 * audio_fmt EMAGE_PCM_S16 (decoded x * 2^-15, what a 16-bit PCM file loads as) or EMAGE_PCM_F32; `clips`: n_clips rows of three 64-bit words
 * {first frame, first sample, recording id (unused here)}.  Batch row b takes clip id = order[p * batch + b] with p = *cursor mod n_batches (cursor:
 * one int32 on the device, so a captured graph walks the epoch; past the epoch's end it wraps to the first batch instead of reading behind the
 * `order` buffer of n_order >= n_batches * batch int32 ids) and copies `frames` rows of each motion array and frames * samples_per_frame samples:
 *   out_audio[b * ld_audio + i];  out_X[b * X_clip_pitch + t * X_row_pitch + c]     (pitches in elements: the outputs may be strided views)
 * Every access is one element at its natural alignment (clips start at any frame and any sample).  An id outside [0, n_clips) zero-fills batch
 * row b and ORs 1 into *status (one int32 on the device, sticky: the caller clears it); a table row that does not lie inside the flat arrays
 * zero-fills likewise and ORs 2.  Nothing outside the arrays is ever read. */
#define EMAGE_CLIP_POSE_DIMS 165
#define EMAGE_CLIP_EXPR_DIMS 100
#define EMAGE_CLIP_TRANS_DIMS 3
#define EMAGE_CLIP_CONTACT_DIMS 4
int emage_gather_clips(const int* order, long n_order, const int* cursor, int n_batches, int batch,
                       const long long* clips, long n_clips, int frames, int samples_per_frame,
                       const float* poses, const float* expressions, const float* trans, const float* contact, long total_frames,
                       int audio_fmt, const void* audio, long total_samples,
                       float* out_audio, long ld_audio,
                       float* out_poses, long poses_clip_pitch, long poses_row_pitch,
                       float* out_expressions, long expressions_clip_pitch, long expressions_row_pitch,
                       float* out_trans, long trans_clip_pitch, long trans_row_pitch,
                       float* out_contact, long contact_clip_pitch, long contact_row_pitch,
                       int* status, void* stream);

/* The random motion mask of train_emage_audio.py:163-165 (torch.rand(bs, t, 337) < mask_ratio, as float) drawn on the device:
 *   out[i] = (u_i < (float)(a * iteration + b)) ? 1 : 0,   u_i = (word >> 8) * 2^-24 of Philox4x32-10
 * with key = seed, counter = (i / 4, mask_id, iteration), element i taking word i % 4 — the convention of emage_dropout_mask.  iteration: one int32
 * on the device (a captured step draws a fresh mask with a fresh ratio at every replay); a * iteration + b is evaluated in double and rounded to
 * fp32 once, as torch rounds the reference's Python float for the comparison.  The ratio is not clamped: above 1 every element is 1. */
int emage_motion_mask(float* out, long n, double a, double b, unsigned long long seed, unsigned mask_id, const int* iteration, void* stream);

/* The speaker-table row of every clip of the batch emage_gather_clips cuts for the same cursor value:
 *   out[b] = speakers[clips[id * 3 + 2]],  id = order[(*cursor mod n_batches) * batch + b]
 * speakers: n_recordings int64 rows (one per recording of the store, >= 0); out: `batch` int64 words.  An id outside [0, n_clips) writes 0 and
 * ORs 1 into *status; a clip whose recording id lies outside [0, n_recordings), or a negative speaker row, writes 0 and ORs 2 (the status word
 * and its meaning are emage_gather_clips').  Nothing outside the three tables is ever read. */
int emage_gather_clip_speakers(const int* order, long n_order, const int* cursor, int n_batches, int batch,
                               const long long* clips, long n_clips, const int64_t* speakers, long n_recordings,
                               int64_t* out, int* status, void* stream);

/* A batch of audio windows cut out of the flat array that holds every recording end to end, in ONE launch (csrc/recordings.hip; the audio
 * slices of EmageAudioModel.inference's windows, M:393-394 / M:441-442, for recordings of different lengths): row b of out (n rows of pitch
 * ld_out >= samples floats) takes `samples` samples starting at offsets[b] (n 64-bit words on the device), audio_fmt EMAGE_PCM_S16 (decoded
 * x * 2^-15) or EMAGE_PCM_F32 as in emage_gather_clips.  Rows may start at any sample of any recording: 16-byte loads from the first aligned
 * sample of the source on, 16-byte stores where the destination is aligned at the same sample, single elements before and behind.  A row with
 * offsets[b] < 0 or offsets[b] + samples > total_samples is zero-filled and ORs 1 into *status (one int32 on the device, sticky); nothing
 * outside the array is ever read. */
int emage_gather_windows(int audio_fmt, const void* audio, long total_samples, const long long* offsets, int n, int samples,
                         float* out, long ld_out, int* status, void* stream);

/* Table-driven row copies between two device buffers of src_rows / dst_rows rows of width_bytes bytes each, in ONE launch: `segments` holds
 * n_segments rows of three 64-bit words {first source row, first destination row, rows} on the device; max_rows: an upper bound of every
 * segment's length (it sizes the grid).  16-byte accesses where source and destination are aligned alike, 4-byte words or single bytes
 * otherwise.  A segment that does not lie inside both buffers, or is longer than max_rows, is skipped and ORs 2 into *status; destination
 * rows no segment names are left as they are.  Segments whose destinations overlap each other or their sources are the caller's error
 * (pantomatrix_amd.ops.segment_table checks a table when it is built). */
int emage_copy_segments(const void* src, long src_rows, void* dst, long dst_rows, const long long* segments, int n_segments,
                        long width_bytes, long max_rows, int* status, void* stream);

/* The streaming batch (csrc/stream.hip; pantomatrix_amd/streaming.py): `slots` live sessions of EmageAudioModel.inference whose audio arrives
 * while they run.  Each entry point is ONE launch over all slots, driven by the per-tick table: EMAGE_STREAM_WORDS int32 words per slot on the
 * device, filled by the host (which knows what it pushed; nothing is read back to build it):
 *   READY        the slot runs a window this tick (0: its state is left bit for bit as it is and its output rows are zero)
 *   AUDIO_READ   position in the slot's audio ring of the window's first sample      AUDIO_WRITE  position where this tick's PCM lands
 *   PUSH_COUNT   samples of this tick's PCM for the slot (0: none)                   PUSH_SRC     their first sample in the staged buffer
 *   CODE_WRITE   position in the slot's code rings of the window's first kept code
 *   SEG_READ     position in the code rings of the decode segment's row 0            SEG_VALID    codes the segment holds from row 0 on
 *   EMIT_ROW     segment row of the first frame to emit                              EMIT_COUNT   frames to emit
 * Rings wrap at any element.  A row that points outside its buffers is skipped — nothing outside the buffers is read or written, the outputs
 * the row would have filled are zero — and ORs EMAGE_STREAM_BAD_* into *status (one int32 on the device, sticky). */
#define EMAGE_STREAM_WORDS 12
#define EMAGE_STREAM_READY 0
#define EMAGE_STREAM_AUDIO_READ 1
#define EMAGE_STREAM_AUDIO_WRITE 2
#define EMAGE_STREAM_PUSH_COUNT 3
#define EMAGE_STREAM_PUSH_SRC 4
#define EMAGE_STREAM_CODE_WRITE 5
#define EMAGE_STREAM_SEG_READ 6
#define EMAGE_STREAM_SEG_VALID 7
#define EMAGE_STREAM_EMIT_ROW 8
#define EMAGE_STREAM_EMIT_COUNT 9
#define EMAGE_STREAM_BAD_PUSH 1
#define EMAGE_STREAM_BAD_WINDOW 2
#define EMAGE_STREAM_BAD_COMMIT 4
#define EMAGE_STREAM_BAD_EMIT 8

/* ring[slot][(AUDIO_WRITE + i) mod ring_len] = staged[PUSH_SRC + i] for i < PUSH_COUNT: the staged buffer (staged_samples samples,
 * EMAGE_PCM_S16 decoded x * 2^-15 as in emage_gather_windows, or EMAGE_PCM_F32) holds the tick's PCM of every slot end to end; ring: (slots,
 * ring_len) fp32.  Skipped (EMAGE_STREAM_BAD_PUSH) unless 0 <= PUSH_COUNT <= ring_len, the source range lies inside the staged buffer and
 * 0 <= AUDIO_WRITE < ring_len. */
int emage_stream_push(int audio_fmt, const void* staged, long staged_samples, const int* table, int slots, float* ring, long ring_len,
                      int* status, void* stream);

/* emage_stream_push for sessions whose PCM arrives at ANY rate and layout: decode, channel mean and the polyphase filter of
 * emage_audio_resample, continued across pushes, in ONE launch over all slots.  The samples a slot's ring receives equal
 * emage_audio_resample over the session's whole PCM bit for bit, wherever the pushes were cut (same taps, same fmaf order: csrc/pcm_taps.h).
 *   formats   HOST array of n_formats (1 .. EMAGE_STREAM_MAX_FORMATS) rows of EMAGE_STREAM_FORMAT_WORDS ints, validated here and carried to
 *             the device by value: PCM code, channels (1..8), up, down (lowest terms of 16000 / rate, each <= 65536), half, rpp, row pitch and
 *             the float offset (a multiple of 4) of the format's phase rows in `taps`.  up != down: half = 10 max(up, down),
 *             rpp = ceil((2 half + 1) / up), pitch = rpp | 1, the rows as emage_audio_resample takes them, within its two LDS budgets.
 *             up == down == 1: decode and channel mean only; half = 0, rpp = 1, pitch = 0, no rows.
 *   taps      the phase rows of every format in one device buffer of taps_floats floats, 16-byte aligned.
 *   staged    the tick's PCM of every slot (staged_bytes bytes, 16-byte aligned); a slot's frames are contiguous from a 16-byte boundary.
 *   history   (slots, 2, hist_len) fp32: per slot two sides of the last hist_len decoded mono frames, the newest last.  hist_len >= rpp - 1
 *             of every format.  A push reads side HIST_SIDE and writes the other; the host flips HIST_SIDE with every push of the slot.
 *   rs_table  EMAGE_STREAM_RS_WORDS int32 words per slot on the device.  Positions are relative, so they fit whatever the session's age:
 *     FRAMES      frames staged for the slot this tick (0: none)          SRC16      their first byte in `staged`, in units of 16 bytes
 *     FORMAT      row of `formats`                                        FINAL      the input has ended: frames behind the staged ones are zeros
 *     OUT_COUNT   outputs to write this tick                              OUT_POS    ring position of the first, m0 mod ring_len
 *     KMAX0       (m0 down + half) / up - (frames pushed before this tick): the newest frame output m0 reads, relative to the first staged one
 *     R0          (m0 down + half) mod up: its phase row
 *     HIST_VALID  frames of the read side that exist (the rest, before the session's start, read as zeros)       HIST_SIDE  the side to read
 *   Output m0 + j reads frames kmax - rpp + 1 .. kmax with kmax = KMAX0 + (j down + R0) / up: negative ones from the history, 0 .. FRAMES - 1
 *   from the staged PCM.  A row with FRAMES and OUT_COUNT both 0 does nothing; FRAMES > 0 always writes the other history side (OUT_COUNT may
 *   be 0); FRAMES == 0 with FINAL only flushes.  Skipped — ring and history untouched, EMAGE_STREAM_BAD_RESAMPLE — is a row with FORMAT
 *   outside `formats`, the staged range outside `staged`, OUT_COUNT outside [0, ring_len], OUT_POS outside [0, ring_len), KMAX0 < 0, R0 outside
 *   [0, up), HIST_VALID outside [0, hist_len], HIST_SIDE not 0 / 1, or — without FINAL — a last output that reads a frame behind the staged ones. */
#define EMAGE_STREAM_RS_WORDS 12
#define EMAGE_STREAM_RS_FRAMES 0
#define EMAGE_STREAM_RS_SRC16 1
#define EMAGE_STREAM_RS_FORMAT 2
#define EMAGE_STREAM_RS_FINAL 3
#define EMAGE_STREAM_RS_OUT_COUNT 4
#define EMAGE_STREAM_RS_OUT_POS 5
#define EMAGE_STREAM_RS_KMAX0 6
#define EMAGE_STREAM_RS_R0 7
#define EMAGE_STREAM_RS_HIST_VALID 8
#define EMAGE_STREAM_RS_HIST_SIDE 9
#define EMAGE_STREAM_BAD_RESAMPLE 16
#define EMAGE_STREAM_MAX_FORMATS 8
#define EMAGE_STREAM_FORMAT_WORDS 8
int emage_stream_push_resample(const void* staged, long staged_bytes, const int* rs_table, int slots, const int* formats, int n_formats,
                               const float* taps, long taps_floats, float* ring, long ring_len, float* history, int hist_len, int* status,
                               void* stream);

/* out[slot][i] = ring[slot][(AUDIO_READ + i) mod ring_len] for i < samples (<= ring_len) when the slot is READY, else 0: the audio slice of a
 * window (M:393-394) as a row of the (slots, samples) batch, pitch ld_out floats.  AUDIO_READ outside [0, ring_len): zero-filled,
 * EMAGE_STREAM_BAD_WINDOW. */
int emage_stream_windows(const float* ring, long ring_len, const int* table, int slots, int samples, float* out, long ld_out, int* status,
                         void* stream);

/* After a window's forward and seed decode.  For a READY slot: code_ring[p][slot][(CODE_WRITE + j) mod ring_codes] = win_codes[p][slot][j] for
 * j < keep (the window's first `keep` of `window` codes, M:419) for each of the `parts` routed parts, and seeds[slot] = the seed_floats floats
 * at new_seed + slot * ld_seed (the last seed frames of the window's decode, M:412-418).  Then, for EVERY slot, the decode segment:
 * segment[p][slot][j] = code_ring[p][slot][(SEG_READ + j) mod ring_codes] for j < SEG_VALID, code 0 for the rows behind and for every row of
 * a slot that is not READY.  win_codes (parts, slots, window), code_ring (parts, slots, ring_codes), segment (parts, slots, seg_len): int64.
 * A READY row with CODE_WRITE or SEG_READ outside [0, ring_codes) or SEG_VALID outside [0, min(seg_len, ring_codes)] is treated as not READY
 * (EMAGE_STREAM_BAD_COMMIT). */
int emage_stream_commit(const int* table, int slots, int parts, const int64_t* win_codes, int window, int keep, int64_t* code_ring,
                        int ring_codes, int64_t* segment, int seg_len, const float* new_seed, long ld_seed, float* seeds, int seed_floats,
                        int* status, void* stream);

/* From the decoded segment (axis_angle (slots * seg_len, 165), expression (slots * seg_len, 100), vel: (slots * seg_len) rows of pitch ldv whose
 * columns col0 .. col0 + 2 are the global model's x velocity, height and z velocity) rows EMIT_ROW .. EMIT_ROW + EMIT_COUNT - 1 of a READY slot
 * go to rows 0 .. EMIT_COUNT - 1 of its (out_rows, .) output rows: poses, expressions, codes[row][p] = segment[p][slot][EMIT_ROW + row], and
 * trans = (x, height, z) with the recurrence of emage_velocity_to_position CONTINUED from carry[slot] (3 floats; x and z are used): the first
 * emitted row takes the carried position, each later one pos = fadd(fmul(v[row - 1], dt), pos), and the position behind the last emitted row is
 * stored back — consecutive calls equal one scan over the whole sequence bit for bit.  Rows behind EMIT_COUNT are zero.  EMIT_COUNT outside
 * [0, out_rows] or rows outside the segment: nothing emitted, carry kept, EMAGE_STREAM_BAD_EMIT. */
int emage_stream_emit(const int* table, int slots, int seg_len, int out_rows, const float* axis_angle, const float* expression, const float* vel,
                      int ldv, int col0, float dt, const int64_t* segment, int parts, float* carry, float* poses, float* expressions,
                      float* trans, int64_t* codes, int* status, void* stream);

/* Motion hints of live sessions (streaming.StreamBatch(motion_hints=True); rule 5 of pantomatrix_amd/streaming.py): ONE launch over all slots
 * moves the tick's staged hint frames into the per-slot hint rings and writes the (slots, 2) int64 table emage_pack_motion_hints reads.
 *   ring_motion (slots, hint_rows + 4, ld) fp32 / ring_keep (same shape) uint8, ld >= 337: frame f of a session lives at row f mod hint_rows,
 *             and rows hint_rows .. hint_rows + 3 MIRROR rows 0 .. 3 (a frame that lands in a row below 4 is written twice), so the 64 rows from
 *             (60 i) mod hint_rows are window i, contiguous, for every i (hint_rows: a multiple of 60, >= 120).  Columns 337 .. ld - 1 of a
 *             written row are 0 (motion) / 1 (keep).
 *   staged    the tick's hint frames of every slot (staged_bytes bytes, 16-byte aligned); a slot's chunk starts at a 16-byte boundary and holds
 *             COUNT rows of W floats, then COUNT rows of 337 mask bytes (1 = generate, 0 = given).  FORM EMAGE_STREAM_HINT_PACKED: W = 337, the
 *             model's layout (55 x rot6d | trans | contact); EMAGE_STREAM_HINT_TRACKER: W = 172 = 165 axis-angle | 3 trans | 4 contact, each
 *             joint converted with emage_axis_angle_to_rot6d's arithmetic, bit for bit.
 *   seeds     (slots, 4, 337) fp32, the seed rows of emage_stream_commit: the first SEED_COUNT staged frames' motion also goes to rows SEED_ROW ..
 *             of the slot's seed (frames 0 .. 3 of a session: window 0's seed, M:379).
 *   hint_table  EMAGE_STREAM_HINT_WORDS int32 words per slot on the device:
 *     COUNT       frames staged for the slot this tick (0: none)        SRC16      their first byte in `staged`, in units of 16 bytes
 *     FORM        EMAGE_STREAM_HINT_PACKED / _TRACKER                   WRITE      ring row of the first staged frame
 *     SEED_ROW    seed row the first staged frame goes to               SEED_COUNT leading staged frames that are seed frames (0: none)
 *     READY       the slot runs a window this tick AND reads hints      WIN_FIRST  ring row of the window's frame 0
 *     WIN_AVAIL   hint frames the window may read from WIN_FIRST on (the frames behind count as masked)
 *   window_table[slot] = {slot (hint_rows + 4) + WIN_FIRST, WIN_AVAIL} for a READY slot — a row of the rings read as ONE store of
 *             slots (hint_rows + 4) rows — and {0, 0} for every other slot: a window without hints.
 * A row is skipped — nothing read, nothing written but window_table[slot] = {0, 0}; EMAGE_STREAM_BAD_HINTS — unless 0 <= COUNT <= hint_rows, the
 * chunk lies inside `staged`, FORM is known, 0 <= WRITE < hint_rows, SEED_COUNT = 0 or (SEED_ROW = WRITE, SEED_ROW + SEED_COUNT <= 4, SEED_COUNT <=
 * COUNT), and when READY 0 <= WIN_AVAIL <= window, 0 <= WIN_FIRST and WIN_FIRST + window <= hint_rows + 4. */
#define EMAGE_STREAM_HINT_WORDS 12
#define EMAGE_STREAM_HINT_COUNT 0
#define EMAGE_STREAM_HINT_SRC16 1
#define EMAGE_STREAM_HINT_FORM 2
#define EMAGE_STREAM_HINT_WRITE 3
#define EMAGE_STREAM_HINT_SEED_ROW 4
#define EMAGE_STREAM_HINT_SEED_COUNT 5
#define EMAGE_STREAM_HINT_READY 6
#define EMAGE_STREAM_HINT_WIN_FIRST 7
#define EMAGE_STREAM_HINT_WIN_AVAIL 8
#define EMAGE_STREAM_HINT_PACKED 0
#define EMAGE_STREAM_HINT_TRACKER 1
#define EMAGE_STREAM_BAD_HINTS 32
int emage_stream_push_hints(const void* staged, long staged_bytes, const int* hint_table, int slots, float* ring_motion, unsigned char* ring_keep,
                            int hint_rows, int ld, float* seeds, long long* window_table, int window, int* status, void* stream);

/* The metrics of one validation step (train_emage_audio.py:130-204, mode="val": get_rec_loss / get_cls_loss of the three eval forwards, the
 * arg-max codes) over the REAL clips of a padded batch, in two launches (csrc/val.hip).  `entries`: a HOST array of up to
 * EMAGE_VAL_MAX_ENTRIES rows, one per (forward, body part), validated here and carried to the device by value in the kernel arguments
 * (nothing a captured graph must keep alive); every pointer in it is device memory:
 *   rec (M, C) fp32 rows of pitch ld_rec, latent (M, C) of pitch ld_latent;  logits (M, K) of pitch ld_logits;  index (M) int64;
 *   pred: NULL, or the int64 arg-max output addressed like idx of emage_argmax_logsoftmax_f32 (pred_rows, pred_ld; pred_rows <= 0: a flat list);
 *   l_w, c_w: the weights of the entry's MSE / NLL in its forward's rec / cls loss;  tag in [0, EMAGE_VAL_TAGS): the forward.
 * T: frames per clip (M % T == 0);  n_valid: one int32 in DEVICE memory, the real clips of the batch (clamped to [0, M / T]).
 * Per row m < n_valid * T of an entry: the fp32 log-softmax over K, NLL at index[m], the arg-max — exactly the index
 * emage_argmax_logsoftmax_f32 returns on the same logits (first maximum on ties, the same rule for NaN rows) —, hit = (arg-max == index[m]),
 * and sum_c (rec - latent)^2 with difference and square in fp32 as emage_mse_loss and the sum in float64.  Rows at or beyond n_valid * T
 * contribute nothing, whatever they hold (NaN, Inf); their pred is still written.  An index outside [0, K) contributes no NLL and no hit
 * and sets the status word (sticky: the caller clears it), the convention of emage_nll_loss.
 * acc: EMAGE_VAL_ACC_WORDS 8-byte words in device memory, float64 [LAST, LAST + 7) and [METER, METER + 7), int64 from HITS on:
 *   last[2 tag] = sum over the tag's entries of l_w * mse (mean over n_valid * T * C), last[2 tag + 1] = sum of c_w * nll (mean over
 *   n_valid * T), last[6] = their sum — the reference's rec_seed, cls_seed, rec_audio, cls_audio, rec_mask, cls_mask, all for tags 0, 1, 2;
 *   meter[k] += last[k];  hits[entry] += its hit count;  rows += n_valid * T;  batches += 1;  status |= 1 on a bad index;
 *   last_hits[entry] / last_rows = this call's hit counts and n_valid * T (the per-batch accuracies beside last[]).
 * n_valid == 0 changes nothing in acc.  Sums are taken in a fixed order (per-block partials in the workspace, no atomics): the same inputs
 * give the same bits in every run and every graph replay.  workspace: emage_val_metrics_workspace_bytes(M, n_entries) bytes, 8-byte aligned.
 * EMAGE_EINVAL before any launch: a NULL entries / n_valid / acc / workspace / rec / latent / logits / index, n_entries outside
 * [1, EMAGE_VAL_MAX_ENTRIES], M <= 0, T <= 0, M % T != 0, K outside [2, EMAGE_VAL_MAX_WIDTH], C outside [1, EMAGE_VAL_MAX_WIDTH] (neither
 * needs to be a multiple of anything), a pitch smaller than its width, a pred view that does not divide M, a tag outside its range, a
 * workspace that is too small, pointers off their natural alignment. */
#define EMAGE_VAL_MAX_ENTRIES 12
#define EMAGE_VAL_MAX_WIDTH 1024
#define EMAGE_VAL_TAGS 3
#define EMAGE_VAL_LOSSES 7
#define EMAGE_VAL_ACC_LAST 0
#define EMAGE_VAL_ACC_METER 7
#define EMAGE_VAL_ACC_HITS 14
#define EMAGE_VAL_ACC_ROWS 26
#define EMAGE_VAL_ACC_BATCHES 27
#define EMAGE_VAL_ACC_STATUS 28
#define EMAGE_VAL_ACC_LAST_HITS 29
#define EMAGE_VAL_ACC_LAST_ROWS 41
#define EMAGE_VAL_ACC_WORDS 48
typedef struct emage_val_entry {
    const float* rec; const float* latent; const float* logits; const int64_t* index; int64_t* pred;
    int ld_rec, ld_latent, ld_logits, C, K, pred_rows, tag;
    long pred_ld;
    double l_w, c_w;
} emage_val_entry;
long emage_val_metrics_workspace_bytes(int M, int n_entries);
int emage_val_metrics(const emage_val_entry* entries, int n_entries, int M, int T, const int* n_valid, void* acc,
                      void* workspace, long workspace_bytes, void* stream);

/*
 * rep15d (csrc/motion_rep.hip): the motion representation the reference's BC / L1div metrics read, emage_utils/motion_rep_transfer.py:51-64,
 * from what this library generates and the joint positions that belong to it.
 *   poses (B * T, 165) fp32 axis-angle, contiguous;  joints (B * T, >= 55, 3) fp32 rows of pitch ld_joints >= 165 floats: the first 55 SMPL-X
 *   joints of each frame (from whatever evaluates the body model);  rep (B, T, 55, 15) fp32, contiguous, per joint
 *   [position 3 | velocity 3 | rot-6D 6 | angular velocity 3].
 * Differences per sequence of T >= 2 frames: (x[1] - x[0]) / dt at the first frame, (x[n + 1] - x[n - 1]) / (2 dt) inside,
 * (x[T - 1] - x[T - 2]) / dt at the last; x = the joint position (velocity) or the pose (angular velocity); fp32 subtraction, then an fp32
 * division.  rot-6D is emage_axis_angle_to_rot6d's arithmetic, bit for bit.  One launch, no frame of another sequence is read.
 * EMAGE_EINVAL before any launch: a NULL pointer, B <= 0, T < 2, ld_joints < 165, dt not positive, B * T beyond the grid limit.
 */
#define EMAGE_REP_JOINTS 55
int emage_motion_rep(const float* poses, const float* joints, long ld_joints, float dt, float* rep, int B, int T, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EMAGE_HIP_H */
