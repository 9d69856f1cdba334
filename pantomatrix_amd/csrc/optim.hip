// The optimizer of the EMAGE training step (pantomatrix_amd/training.py), on flat fp32 tensors:
//   emage_adam_step / emage_adam_step_dev   torch.optim.Adam for one tensor; the step count given by the host, or read from device memory
//   emage_adam_multi / emage_adam_multi_scaled (+ emage_adam_multi_chunk)   every tensor of a table in one launch
//   emage_grad_sumsq_multi (+ emage_grad_norm_workspace_bytes) / emage_scale_multi   global gradient norm and clipping over the same table
// One element update (adam_update), one pair of bias-correction coefficients (adam_coeffs) and one table decode (adam_table_chunk) serve
// all of them.  The forward pieces and losses are in train.hip, the backward kernels in train_backward.hip.
#include "col_reduce.h"
#include <math.h>

namespace {

// torch.optim.Adam (no amsgrad, weight decay folded into the gradient when non-zero), T:258-265:
//   m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g g;  p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
// The coefficients of step t.  emage_adam_step evaluates them on the host, the kernels that read t from device memory on the device: the
// two `pow` are different libraries and are not known to agree for every t, so each entry point keeps its place of evaluation.
struct AdamCoeffs { float step_size, inv_sqrt_bias2; };
__host__ __device__ inline AdamCoeffs adam_coeffs(float lr, float b1, float b2, int t) {
    const double bias1 = 1.0 - pow((double)b1, t), bias2 = 1.0 - pow((double)b2, t);
    return {(float)((double)lr / bias1), (float)(1.0 / sqrt(bias2))};
}

// element i with its (already scaled) gradient gi
__device__ __forceinline__ void adam_update(float* __restrict__ p, float* __restrict__ m, float* __restrict__ v, long i, float gi,
                                            float b1, float b2, AdamCoeffs k, float eps, float weight_decay) {
    if (weight_decay != 0.f) gi += weight_decay * p[i];
    const float mi = b1 * m[i] + (1.f - b1) * gi;
    const float vi = b2 * v[i] + (1.f - b2) * gi * gi;
    m[i] = mi;
    v[i] = vi;
    p[i] -= k.step_size * mi / (sqrtf(vi) * k.inv_sqrt_bias2 + eps);
}

__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long n,
                                                   float b1, float b2, AdamCoeffs k, float eps, float weight_decay) {
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) adam_update(p, m, v, i, g[i], b1, b2, k, eps, weight_decay);
}

// the step count read from device memory (a captured hipGraph replays with fixed kernel arguments: the count must advance on the device)
__global__ __launch_bounds__(256) void adam_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, long n,
                                                       const int* __restrict__ step, float lr, float b1, float b2, float eps, float weight_decay) {
    const AdamCoeffs k = adam_coeffs(lr, b1, b2, *step);
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) adam_update(p, m, v, i, g[i], b1, b2, k, eps, weight_decay);
}

// ---- multi-tensor Adam -----------------------------------------------------------------------------------------------------------------
// ONE launch for every parameter of the model instead of one per tensor (445 launches): `table` holds, per tensor, the five 64-bit words
// {param, grad, exp_avg, exp_avg_sq, n}; block b works on chunk block_chunk[b] (ADAM_CHUNK elements) of tensor block_tensor[b].
// grad_scale multiplies every gradient first (the 1 / world_size of the data-parallel average); with zero_grad the gradient is cleared
// behind the update (the next step accumulates into it again).
constexpr int ADAM_CHUNK = 4096;
struct AdamChunk { float* p; float* g; float* m; float* v; long i0, i1; };          // the tensor of this block and its element range [i0, i1)
__device__ __forceinline__ AdamChunk adam_table_chunk(const long long* __restrict__ table, const int* __restrict__ block_tensor, const int* __restrict__ block_chunk) {
    const long long* e = table + 5 * (long)block_tensor[blockIdx.x];
    const long n = (long)e[4];
    const long i0 = (long)block_chunk[blockIdx.x] * ADAM_CHUNK;
    return {(float*)e[0], (float*)e[1], (float*)e[2], (float*)e[3], i0, i0 + ADAM_CHUNK < n ? i0 + ADAM_CHUNK : n};
}

__global__ __launch_bounds__(256) void adam_multi_kernel(const long long* __restrict__ table, const int* __restrict__ block_tensor, const int* __restrict__ block_chunk,
                                                         const int* __restrict__ step_dev, int step, float lr, float b1, float b2, float eps, float weight_decay,
                                                         float grad_scale, int zero_grad, const int* __restrict__ skip,
                                                         const float* __restrict__ grad_scale_dev) {
    if (grad_scale_dev) grad_scale = grad_scale * *grad_scale_dev;      // the clip coefficient of emage_grad_sumsq_multi: one fp32 product per block
    const bool skipped = skip && *skip != 0;             // a non-finite gradient was counted: parameters and moments stay as they are
    const AdamCoeffs k = adam_coeffs(lr, b1, b2, step_dev ? *step_dev : step);
    const AdamChunk t = adam_table_chunk(table, block_tensor, block_chunk);
    float* __restrict__ g = t.g;
    if (skipped) {
        if (zero_grad)
            for (long i = t.i0 + threadIdx.x; i < t.i1; i += 256) g[i] = 0.f;
        return;
    }
    for (long i = t.i0 + threadIdx.x; i < t.i1; i += 256) {
        adam_update(t.p, t.m, t.v, i, g[i] * grad_scale, b1, b2, k, eps, weight_decay);
        if (zero_grad) g[i] = 0.f;
    }
}

// ---- global gradient norm and clipping -----------------------------------------------------------------------------------------------
// torch.nn.utils.clip_grad_norm_ (norm_type 2) over the gradients of an Adam table (the layout of emage_adam_multi), INSIDE the step: the
// norm is needed between the gradient exchange and Adam, a window a captured step only has on the device.  Two launches, every sum in
// float64 with a fixed order (no atomics: the same input gives the same bits):
//   sumsq_partial_kernel   block b -> partial[b] = sum of g^2 over its ADAM_CHUNK elements.  Each g is squared as a double (the product of
//                          two 24-bit significands is exact; an fp32 square would flush below 1e-19 and overflow above 1e19).  Thread j adds
//                          elements j, j + 256, ... in order; 64 lanes by a shuffle tree; the 4 wave sums in order.  Plain dword loads: the
//                          gradients are bucket views with 4-byte alignment only, a wave reads 256 contiguous bytes per instruction, and the
//                          order of the sum does not depend on where the view starts.
//   sumsq_finalize_kernel  ONE block of 1024 threads.  Wave w adds the partials of tensors w, w + 16, ... (lane l: partials l, l + 64, ...
//                          of the tensor in order, then the shuffle tree) -> tensor_sumsq[t]; then thread j adds its contiguous range of
//                          tensors in table order, a shared-memory tree adds the 1024 thread sums -> total, norm and the clip coefficient.
// The blocks of a tensor are consecutive in block_tensor with ascending chunks (as every table of this library is built): the block of
// chunk 0 records where the tensor's partials start.
constexpr int NORM_FIN_THREADS = 1024;
__global__ __launch_bounds__(256) void sumsq_partial_kernel(const long long* __restrict__ table, const int* __restrict__ block_tensor,
                                                            const int* __restrict__ block_chunk, double* __restrict__ partial, int* __restrict__ first_block) {
    __shared__ double red[4];
    const AdamChunk t = adam_table_chunk(table, block_tensor, block_chunk);
    const float* __restrict__ g = t.g;
    double s = 0.0;
#pragma unroll 4
    for (long i = t.i0 + threadIdx.x; i < t.i1; i += 256) {
        const double v = (double)g[i];
        s += v * v;
    }
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
        if (block_chunk[blockIdx.x] == 0) first_block[block_tensor[blockIdx.x]] = (int)blockIdx.x;
    }
}
__global__ __launch_bounds__(NORM_FIN_THREADS) void sumsq_finalize_kernel(const long long* __restrict__ table, const double* __restrict__ partial,
                                                                          const int* __restrict__ first_block, int n_blocks, int n_tensors, double pre_scale,
                                                                          double max_norm, double* __restrict__ tensor_sumsq, double* __restrict__ total_sumsq,
                                                                          float* __restrict__ norm, float* __restrict__ coef) {
    __shared__ double red[NORM_FIN_THREADS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int t = wave; t < n_tensors; t += NORM_FIN_THREADS / 64) {
        const long n = (long)table[5 * (long)t + 4];
        const long nb = n > 0 ? (n + ADAM_CHUNK - 1) / ADAM_CHUNK : 0;
        double s = 0.0;
        if (nb > 0) {
            const long first = first_block[t];
            if (first < 0 || first + nb > n_blocks) s = NAN;          // a table whose blocks are not laid out as described above
            else
                for (long k = lane; k < nb; k += 64) s += partial[first + k];
        }
        s = wave_sum(s);
        if (lane == 0) tensor_sumsq[t] = s;
    }
    __syncthreads();                                      // tensor_sumsq was written by this block: visible to all of its threads from here on
    const int per = (n_tensors + NORM_FIN_THREADS - 1) / NORM_FIN_THREADS;
    const int t0 = threadIdx.x * per, t1 = t0 + per < n_tensors ? t0 + per : n_tensors;
    double a = 0.0;
    for (int t = t0; t < t1; ++t) a += tensor_sumsq[t];
    red[threadIdx.x] = a;
    const double total = block_tree_sum<NORM_FIN_THREADS>(red);
    if (threadIdx.x == 0) {
        const double nrm = pre_scale * sqrt(total);
        *total_sumsq = total;
        *norm = (float)nrm;
        double cf = 1.0;
        if (max_norm > 0.0 && !isinf(max_norm)) {
            cf = max_norm / (nrm + 1e-6);                 // torch: clip_coef = max_norm / (total_norm + 1e-6), clamped to at most 1 (a NaN stays a NaN)
            if (cf > 1.0) cf = 1.0;
        }
        *coef = (float)cf;
    }
}
__global__ __launch_bounds__(256) void scale_multi_kernel(const long long* __restrict__ table, const int* __restrict__ block_tensor,
                                                          const int* __restrict__ block_chunk, const float* __restrict__ coef) {
    const float c = *coef;
    const AdamChunk t = adam_table_chunk(table, block_tensor, block_chunk);
    float* __restrict__ g = t.g;
    for (long i = t.i0 + threadIdx.x; i < t.i1; i += 256) g[i] *= c;
}
static inline long norm_workspace_bytes(long n_blocks, long n_tensors) { return 8 * n_blocks + 4 * ((n_tensors + 1) & ~1L); }

}  // namespace

extern "C" int emage_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, int step,
                               float lr, float beta1, float beta2, float eps, float weight_decay, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || n <= 0 || step <= 0 || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) return EMAGE_EINVAL;
    hipLaunchKernelGGL(adam_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, n, beta1, beta2,
                       adam_coeffs(lr, beta1, beta2, step), eps, weight_decay);
    return launch_status();
}

extern "C" int emage_adam_step_dev(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, long n, const int* step,
                                   float lr, float beta1, float beta2, float eps, float weight_decay, void* stream) {
    if (!param || !grad || !exp_avg || !exp_avg_sq || !step || n <= 0 || !(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) return EMAGE_EINVAL;
    hipLaunchKernelGGL(adam_dev_kernel, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, param, grad, exp_avg, exp_avg_sq, n, step, lr, beta1, beta2, eps, weight_decay);
    return launch_status();
}

extern "C" int emage_adam_multi_chunk(void) { return ADAM_CHUNK; }

extern "C" int emage_adam_multi(const long long* table, const int* block_tensor, const int* block_chunk, int n_blocks, const int* step_dev, int step,
                                float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale, int zero_grad, const int* skip,
                                void* stream) {
    return emage_adam_multi_scaled(table, block_tensor, block_chunk, n_blocks, step_dev, step, lr, beta1, beta2, eps, weight_decay, grad_scale, nullptr,
                                   zero_grad, skip, stream);
}

extern "C" int emage_adam_multi_scaled(const long long* table, const int* block_tensor, const int* block_chunk, int n_blocks, const int* step_dev, int step,
                                       float lr, float beta1, float beta2, float eps, float weight_decay, float grad_scale, const float* grad_scale_dev,
                                       int zero_grad, const int* skip, void* stream) {
    if (!table || !block_tensor || !block_chunk || n_blocks <= 0 || (!step_dev && step <= 0)) return EMAGE_EINVAL;
    if (!(beta1 >= 0.f && beta1 < 1.f) || !(beta2 >= 0.f && beta2 < 1.f)) return EMAGE_EINVAL;
    hipLaunchKernelGGL(adam_multi_kernel, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, table, block_tensor, block_chunk, step_dev, step,
                       lr, beta1, beta2, eps, weight_decay, grad_scale, zero_grad, skip, grad_scale_dev);
    return launch_status();
}

extern "C" long emage_grad_norm_workspace_bytes(int n_blocks, int n_tensors) {
    if (n_blocks <= 0 || n_tensors <= 0) return 0;
    return norm_workspace_bytes(n_blocks, n_tensors);
}

extern "C" int emage_grad_sumsq_multi(const long long* table, const int* block_tensor, const int* block_chunk, int n_blocks, int n_tensors,
                                      double pre_scale, double max_norm, double* tensor_sumsq, double* total_sumsq, float* norm, float* coef,
                                      void* workspace, long workspace_bytes, void* stream) {
    if (!table || !block_tensor || !block_chunk || n_blocks <= 0 || n_tensors <= 0 || !tensor_sumsq || !total_sumsq || !norm || !coef) return EMAGE_EINVAL;
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < norm_workspace_bytes(n_blocks, n_tensors)) return EMAGE_EINVAL;
    if (!(pre_scale >= 0.0) || isinf(pre_scale) || max_norm != max_norm) return EMAGE_EINVAL;
    double* partial = (double*)workspace;
    int* first_block = (int*)(partial + n_blocks);
    hipLaunchKernelGGL(sumsq_partial_kernel, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, table, block_tensor, block_chunk, partial, first_block);
    hipLaunchKernelGGL(sumsq_finalize_kernel, dim3(1), dim3(NORM_FIN_THREADS), 0, (hipStream_t)stream, table, partial, first_block, n_blocks, n_tensors,
                       pre_scale, max_norm, tensor_sumsq, total_sumsq, norm, coef);
    return launch_status();
}

extern "C" int emage_scale_multi(const long long* table, const int* block_tensor, const int* block_chunk, int n_blocks, const float* coef, void* stream) {
    if (!table || !block_tensor || !block_chunk || n_blocks <= 0 || !coef) return EMAGE_EINVAL;
    hipLaunchKernelGGL(scale_multi_kernel, dim3(n_blocks), dim3(256), 0, (hipStream_t)stream, table, block_tensor, block_chunk, coef);
    return launch_status();
}
