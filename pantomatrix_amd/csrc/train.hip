// Train-mode forward pieces and losses of the EMAGE training step (reference train_emage_audio.py:130-204 and the
// train-mode behaviour of torch's modules inside models/emage_audio):
//   emage_bn_stats     nn.BatchNorm1d in training mode, statistics half: per-channel batch mean and BIASED variance over all
//                      rows (= B * L positions) of a channels-last conv output, plus the running-statistic update
//                      (momentum, UNBIASED variance) — processing_emage_audio.py:262-294 with nn.BatchNorm1d semantics
//   emage_bn_apply     the normalisation half fused with what follows it inside BasicBlock.forward (P:283-294): affine,
//                      optional shortcut (raw, or itself batch-normalised: the downsample branch), LeakyReLU
//   emage_mul_add      out = a * mask (+ b): nn.Dropout with a given mask (x * bernoulli / (1 - p)) and the residual add that
//                      follows it in nn.Transformer*Layer; the mask may be stored (T, B, d) while rows run (B, T)
//   emage_dropout_mask / emage_mul_add_philox   the mask drawn on the device (Philox4x32-10), stored or applied in place
//   emage_mse_loss / emage_nll_loss   the two loss forms of train_emage_audio.py:106-130, accumulated into a float64 device scalar
//   emage_mse_loss_grad / emage_nll_loss_grad   their gradients with respect to the prediction / the logits
// Statistics are accumulated in float64 (one rounding to fp32 at the end): the batch has up to ~4e5 rows per channel.
// The backward kernels are in train_backward.hip, the optimizer in optim.hip, the float64 reduction pieces all three share in col_reduce.h.
#include "col_reduce.h"
#include "philox.h"
#include <math.h>

namespace {

// partial[(chunk * 2 + {0: sum, 1: sum of squares}) * C + c], deterministic: the finalize kernel adds the chunks in a fixed order
__global__ __launch_bounds__(256) void bn_partial_kernel(const float* __restrict__ x, int ldx, int M, int C, double* __restrict__ partial, int chunk_rows) {
    column_partials<2>(M, C, chunk_rows, partial, [=](long r, int c, double (&s)[2]) {
        const double v = (double)x[r * ldx + c];
        s[0] += v;
        s[1] += v * v;
    });
}

__global__ __launch_bounds__(256) void bn_finalize_kernel(const double* __restrict__ partial, int chunks, int M, int C,
                                                          float* __restrict__ mean, float* __restrict__ var,
                                                          float* __restrict__ running_mean, float* __restrict__ running_var, float momentum) {
    double tot[2];
    int c;
    if (!finalize_sums<2>(partial, chunks, C, blockIdx.x, tot, c)) return;
    const double s = tot[0], ss = tot[1];
    const double mu = s / M;
    double vb = ss / M - mu * mu;
    if (vb < 0.0) vb = 0.0;
    mean[c] = (float)mu;
    var[c] = (float)vb;
    if (running_mean) running_mean[c] = (float)((1.0 - momentum) * running_mean[c] + momentum * (float)mu);
    if (running_var) running_var[c] = (float)((1.0 - momentum) * running_var[c] + momentum * (float)(M > 1 ? vb * M / (M - 1) : vb));
}

struct BnSide { const float* x; int ld; const float* mean; const float* var; const float* gamma; const float* beta; };

// out = leaky(bn(a) + shortcut, slope);  shortcut: none | s.x raw (s.mean == nullptr) | bn(s)
__global__ __launch_bounds__(256) void bn_apply_kernel(BnSide a, BnSide s, float eps, float slope, float* __restrict__ out, int ldo, int M, int C) {
    const long total = (long)M * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long m = i / C;
        const int c = (int)(i - m * C);
        // torch's batch_norm: (x - mean) * invstd * weight + bias, invstd = 1 / sqrt(var + eps)
        float v = (a.x[m * a.ld + c] - a.mean[c]) * (1.0f / sqrtf(a.var[c] + eps)) * a.gamma[c] + a.beta[c];
        if (s.x) {
            float r = s.x[m * s.ld + c];
            if (s.mean) r = (r - s.mean[c]) * (1.0f / sqrtf(s.var[c] + eps)) * s.gamma[c] + s.beta[c];
            v += r;
        }
        out[m * ldo + c] = leaky(v, slope);
    }
}

__global__ __launch_bounds__(256) void mul_add_kernel(const float* __restrict__ a, int lda, const float* __restrict__ mask, int ldm, int t_rows,
                                                      const float* __restrict__ b, int ldb, float* __restrict__ out, int ldo, int M, int C) {
    const long total = (long)M * C;
    const int nb = t_rows > 0 ? M / t_rows : 0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long m = i / C;
        const int c = (int)(i - m * C);
        const long mr = t_rows > 0 ? (m % t_rows) * nb + m / t_rows : m;          // row (b, t) of the stream <-> row (t, b) of the mask
        float v = a[m * lda + c] * mask[mr * ldm + c];
        if (b) v += b[m * ldb + c];
        out[m * ldo + c] = v;
    }
}

// ---- losses (train_emage_audio.py:106-130): block partials in float64, added in block order by one thread -> deterministic

__global__ __launch_bounds__(256) void sq_diff_partial_kernel(const float* __restrict__ a, int lda, const float* __restrict__ b, int ldb, int M, int C,
                                                              double* __restrict__ partial) {
    __shared__ double red[256];
    const long total = (long)M * C;
    double s = 0.0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long m = i / C;
        const int c = (int)(i - m * C);
        const float d = a[m * lda + c] - b[m * ldb + c];          // fp32 difference and square as torch's mse_loss, float64 sum
        s += (double)(d * d);
    }
    red[threadIdx.x] = s;
    const double sum = block_tree_sum<256>(red);
    if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

// -log_softmax(logits[m])[index[m]] summed over the block's rows: one thread per row
__global__ __launch_bounds__(256) void nll_partial_kernel(const float* __restrict__ logits, int ld, const int64_t* __restrict__ index, int M, int K,
                                                          double* __restrict__ partial, int* __restrict__ bad) {
    __shared__ double red[256];
    double s = 0.0;
    for (long m = (long)blockIdx.x * blockDim.x + threadIdx.x; m < M; m += (long)gridDim.x * blockDim.x) {
        const float* x = logits + m * ld;
        float mx = -INFINITY;
        for (int k = 0; k < K; ++k) mx = fmaxf(mx, x[k]);
        float se = 0.f;
        for (int k = 0; k < K; ++k) se += expf(x[k] - mx);
        const int64_t t = index[m];
        if (t < 0 || t >= K) { *bad = 1; continue; }
        s += (double)(-(x[t] - mx - logf(se)));
    }
    red[threadIdx.x] = s;
    const double sum = block_tree_sum<256>(red);
    if (threadIdx.x == 0) partial[blockIdx.x] = sum;
}

__global__ void loss_finalize_kernel(const double* __restrict__ partial, int blocks, double scale, double* __restrict__ loss) {
    double s = 0.0;
    for (int i = 0; i < blocks; ++i) s += partial[i];
    loss[0] += s * scale;
}

__global__ __launch_bounds__(256) void mse_grad_kernel(const float* __restrict__ pred, int ldp, const float* __restrict__ target, int ldt, float scale,
                                                       float* __restrict__ out, int ldo, int M, int C) {
    const long total = (long)M * C;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long m = i / C;
        const int c = (int)(i - m * C);
        out[m * ldo + c] = scale * (pred[m * ldp + c] - target[m * ldt + c]);
    }
}

// out[m][k] = scale * (softmax(logits[m])[k] - [k == index[m]]): one wave per row
__global__ __launch_bounds__(256) void nll_grad_kernel(const float* __restrict__ logits, int ld, const int64_t* __restrict__ index, float scale,
                                                       float* __restrict__ out, int ldo, int M, int K) {
    const int lane = threadIdx.x & 63;
    const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= M) return;
    const float* x = logits + m * ld;
    float mx = -INFINITY;
    for (int k = lane; k < K; k += 64) mx = fmaxf(mx, x[k]);
    for (int o = 32; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
    float se = 0.f;
    for (int k = lane; k < K; k += 64) se += expf(x[k] - mx);
    for (int o = 32; o > 0; o >>= 1) se += __shfl_xor(se, o);
    const int64_t t = index[m];
    for (int k = lane; k < K; k += 64) out[m * ldo + k] = scale * (expf(x[k] - mx) / se - (k == t ? 1.f : 0.f));
}

// ---- device-side dropout masks -------------------------------------------------------------------------------------------------------
// nn.Dropout's keep mask drawn ON THE DEVICE: out[i] = bernoulli(1 - p) / (1 - p) from Philox4x32-10 (Salmon et al., SC'11), a
// counter-based generator, so a mask is a pure function of (seed, step, mask id, element index) — no generator state to carry, no
// host tensors, safe inside a captured hipGraph (the step is read from device memory):
//   key = (seed lo, seed hi);  counter = (i / 4 lo, i / 4 hi, mask id, step);  element i takes word i % 4 of the block;
//   keep  <=>  (word >> 8) * 2^-24 >= p      (24 random bits, uniform on [0, 1))
// The stream is this library's own (documented here, pinned bit for bit by tests/test_train_rng.py against a numpy Philox); it is
// NOT torch's fused-dropout stream: runs are reproducible for a seed, distribution-identical to the reference, not draw-identical.
// The generator itself, philox4x32_10, is in philox.h (data.hip draws the motion mask from it too).
// out = a * keep (+ b) with the keep mask DRAWN IN PLACE: element (mask row mr, column c) is element mr * C + c of the mask
// dropout_mask_kernel would have written for the same key — the same bits as emage_dropout_mask + emage_mul_add, without the mask in
// memory (a training forward holds ~0.9 GB of (T, B, d) masks for its backward otherwise; the backward draws them again from the key).
__global__ __launch_bounds__(256) void mul_add_philox_kernel(const float* __restrict__ a, int lda, float p, float keep_value, unsigned seed_lo, unsigned seed_hi,
                                                             unsigned mask_id, const int* __restrict__ step_dev, int step, int t_rows,
                                                             const float* __restrict__ b, int ldb, float* __restrict__ out, int ldo, int M, int C) {
    const unsigned st = step_dev ? (unsigned)*step_dev : (unsigned)step;
    const int c4 = C >> 2;
    const long total = (long)M * c4;
    const int nb = t_rows > 0 ? M / t_rows : 0;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long m = i / c4;
        const int cq = (int)(i - m * c4);
        const long mr = t_rows > 0 ? (m % t_rows) * nb + m / t_rows : m;          // row (b, t) of the stream <-> row (t, b) of the mask
        const long blk = mr * c4 + cq;                                             // (mr * C + 4 cq) / 4
        unsigned c[4] = {(unsigned)blk, (unsigned)(blk >> 32), mask_id, st};
        philox4x32_10(c, seed_lo, seed_hi);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float k = ((float)(c[e] >> 8) * (1.0f / 16777216.0f) >= p) ? keep_value : 0.f;
            float v = a[m * lda + 4 * cq + e] * k;
            if (b) v += b[m * ldb + 4 * cq + e];
            out[m * ldo + 4 * cq + e] = v;
        }
    }
}
__global__ __launch_bounds__(256) void dropout_mask_kernel(float* __restrict__ out, long n, float p, float keep_value,
                                                           unsigned seed_lo, unsigned seed_hi, unsigned mask_id, const int* __restrict__ step_dev, int step) {
    const unsigned st = step_dev ? (unsigned)*step_dev : (unsigned)step;
    const long nblk = (n + 3) >> 2;
    for (long b = (long)blockIdx.x * blockDim.x + threadIdx.x; b < nblk; b += (long)gridDim.x * blockDim.x) {
        unsigned c[4] = {(unsigned)b, (unsigned)(b >> 32), mask_id, st};
        philox4x32_10(c, seed_lo, seed_hi);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long i = 4 * b + e;
            if (i < n) out[i] = ((float)(c[e] >> 8) * (1.0f / 16777216.0f) >= p) ? keep_value : 0.f;
        }
    }
}

}  // namespace

extern "C" long emage_bn_stats_workspace_bytes(int M, int C) {
    if (M <= 0 || C <= 0) return EMAGE_EINVAL;
    return (long)((M + STAT_CHUNK - 1) / STAT_CHUNK) * 2 * C * (long)sizeof(double);
}

extern "C" int emage_bn_stats(const float* x, int ldx, int M, int C, void* workspace, long workspace_bytes,
                              float* mean, float* var, float* running_mean, float* running_var, float momentum, void* stream) {
    if (!x || !workspace || !mean || !var || M <= 0 || C <= 0 || ldx < C || !(momentum >= 0.f && momentum <= 1.f)) return EMAGE_EINVAL;
    if (workspace_bytes < emage_bn_stats_workspace_bytes(M, C) || ((uintptr_t)workspace & 7)) return EMAGE_EINVAL;
    const int chunk_rows = stat_rows(M), chunks = (M + chunk_rows - 1) / chunk_rows;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bn_partial_kernel, dim3(chunks, (C + 63) / 64), dim3(256), 0, s, x, ldx, M, C, (double*)workspace, chunk_rows);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(bn_finalize_kernel, fin_grid(C), dim3(FIN_THREADS), 0, s, (const double*)workspace, chunks, M, C, mean, var, running_mean, running_var, momentum);
    return launch_status();
}

extern "C" int emage_bn_apply(const float* x, int ldx, const float* mean, const float* var, const float* gamma, const float* beta,
                              const float* sc, int ld_sc, const float* sc_mean, const float* sc_var, const float* sc_gamma, const float* sc_beta,
                              float eps, float slope, float* out, int ldo, int M, int C, void* stream) {
    if (!x || !mean || !var || !gamma || !beta || !out || M <= 0 || C <= 0 || ldx < C || ldo < C || (sc && ld_sc < C)) return EMAGE_EINVAL;
    if (sc_mean && (!sc || !sc_var || !sc_gamma || !sc_beta)) return EMAGE_EINVAL;
    const BnSide a{x, ldx, mean, var, gamma, beta}, s{sc, ld_sc, sc_mean, sc_var, sc_gamma, sc_beta};
    hipLaunchKernelGGL(bn_apply_kernel, dim3(grid_for((long)M * C)), dim3(256), 0, (hipStream_t)stream, a, s, eps, slope, out, ldo, M, C);
    return launch_status();
}

extern "C" int emage_mul_add(const float* a, int lda, const float* mask, int ld_mask, int mask_t_rows, const float* b, int ldb,
                             float* out, int ldo, int M, int C, void* stream) {
    if (!a || !mask || !out || M <= 0 || C <= 0 || lda < C || ld_mask < C || ldo < C || (b && ldb < C)) return EMAGE_EINVAL;
    if (mask_t_rows < 0 || (mask_t_rows > 0 && M % mask_t_rows != 0)) return EMAGE_EINVAL;
    hipLaunchKernelGGL(mul_add_kernel, dim3(grid_for((long)M * C)), dim3(256), 0, (hipStream_t)stream, a, lda, mask, ld_mask, mask_t_rows, b, ldb, out, ldo, M, C);
    return launch_status();
}

extern "C" int emage_mse_loss(const float* pred, int ld_pred, const float* target, int ld_target, int M, int C, float weight,
                              double* loss, void* workspace, void* stream) {
    if (!pred || !target || !loss || !workspace || M <= 0 || C <= 0 || ld_pred < C || ld_target < C || ((uintptr_t)workspace & 7) || ((uintptr_t)loss & 7)) return EMAGE_EINVAL;
    const int blocks = loss_grid((long)M * C);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(sq_diff_partial_kernel, dim3(blocks), dim3(256), 0, s, pred, ld_pred, target, ld_target, M, C, (double*)workspace);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(1), 0, s, (const double*)workspace, blocks, (double)weight / ((double)M * C), loss);
    return launch_status();
}

extern "C" int emage_nll_loss(const float* logits, int ld, const int64_t* index, int M, int K, float weight, double* loss, void* workspace, void* stream) {
    if (!logits || !index || !loss || !workspace || M <= 0 || K <= 0 || ld < K || ((uintptr_t)workspace & 7) || ((uintptr_t)loss & 7)) return EMAGE_EINVAL;
    const int blocks = loss_grid(M);
    hipStream_t s = (hipStream_t)stream;
    int* bad = (int*)((double*)workspace + (LOSS_BLOCKS - 1));                 // last workspace slot: out-of-range class index seen (sticky:
                                                                               // the caller hands in a zeroed workspace, ops.loss_workspace)
    hipLaunchKernelGGL(nll_partial_kernel, dim3(blocks), dim3(256), 0, s, logits, ld, index, M, K, (double*)workspace, bad);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(1), 0, s, (const double*)workspace, blocks, (double)weight / (double)M, loss);
    return launch_status();
}

extern "C" int emage_mse_loss_grad(const float* pred, int ld_pred, const float* target, int ld_target, int M, int C, float weight,
                                   float* grad, int ld_grad, void* stream) {
    if (!pred || !target || !grad || M <= 0 || C <= 0 || ld_pred < C || ld_target < C || ld_grad < C) return EMAGE_EINVAL;
    hipLaunchKernelGGL(mse_grad_kernel, dim3(grid_for((long)M * C)), dim3(256), 0, (hipStream_t)stream, pred, ld_pred, target, ld_target,
                       (float)(2.0 * (double)weight / ((double)M * C)), grad, ld_grad, M, C);
    return launch_status();
}

extern "C" int emage_nll_loss_grad(const float* logits, int ld, const int64_t* index, int M, int K, float weight, float* grad, int ld_grad, void* stream) {
    if (!logits || !index || !grad || M <= 0 || K <= 0 || ld < K || ld_grad < K) return EMAGE_EINVAL;
    hipLaunchKernelGGL(nll_grad_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, logits, ld, index, (float)((double)weight / M), grad, ld_grad, M, K);
    return launch_status();
}

extern "C" int emage_dropout_mask(float* out, long n, float p, unsigned long long seed, unsigned mask_id, const int* step_dev, int step, void* stream) {
    if (!out || n <= 0 || !(p >= 0.f && p < 1.f)) return EMAGE_EINVAL;
    hipLaunchKernelGGL(dropout_mask_kernel, dim3(grid_for((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream, out, n, p, 1.0f / (1.0f - p),
                       (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), mask_id, step_dev, step);
    return launch_status();
}

extern "C" int emage_mul_add_philox(const float* a, int lda, float p, unsigned long long seed, unsigned mask_id, const int* step_dev, int step, int mask_t_rows,
                                    const float* b, int ldb, float* out, int ldo, int M, int C, void* stream) {
    if (!a || !out || M <= 0 || C <= 0 || C % 4 || lda < C || ldo < C || (b && ldb < C) || !(p >= 0.f && p < 1.f) || (mask_t_rows > 0 && M % mask_t_rows)) return EMAGE_EINVAL;
    hipLaunchKernelGGL(mul_add_philox_kernel, dim3(grid_for((long)M * (C / 4))), dim3(256), 0, (hipStream_t)stream, a, lda, p, 1.0f / (1.0f - p),
                       (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), mask_id, step_dev, step, mask_t_rows, b, ldb, out, ldo, M, C);
    return launch_status();
}
