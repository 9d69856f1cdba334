// Quantizer.forward's TRAINING arithmetic (P:144-156) behind the arg-min of vq.hip: the selected codebook rows, the code
// histogram and the two scalars (embedding_loss, perplexity) on the device; the straight-through / commitment backward and
// the codebook gradient.  Every floating-point sum has a fixed order (no floating-point atomics): results are
// bit-reproducible run to run.  The histogram uses integer atomics, which are order-independent.
#include "common.h"
#include "h2.h"
#include <math.h>

namespace {

constexpr int QT_ROWS = 16;        // rows of z per block of vq_quantize_train (4 waves x 4 rows)

__device__ __forceinline__ int clamp_code(long k, int K) { return k < 0 ? 0 : (k >= K ? K - 1 : (int)k); }

__device__ __forceinline__ double wave_sum(double v) {
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);      // xor butterfly: the same association in every lane, every run
    return v;
}

// Block b owns rows [16 b, 16 b + 16): wave w takes rows w, w + 4, ...; a lane walks columns lane, lane + 64, ...
// z_q (fp32) and, when asked, the decoder's operand image (fp32 / bf16 / EMAGE_H2, columns [D, n_store) zero) are written,
// hist[idx[n]] is counted, and sum (e - z)^2 of the block's rows is left in partials[b] as a float64.
template <typename T, bool H2IMG>
__global__ __launch_bounds__(256) void vq_quantize_train(const float* __restrict__ z, int ldz, const float* __restrict__ cb,
                                                         const int64_t* __restrict__ idx, float* __restrict__ zq, int ldo,
                                                         T* __restrict__ img, int ld_img, int n_store, float h2s,
                                                         int* __restrict__ hist, double* __restrict__ partials, int N, int K, int D) {
    __shared__ double s_part[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double acc = 0.0;
    for (int r = wave; r < QT_ROWS; r += 4) {
        const int row = blockIdx.x * QT_ROWS + r;
        if (row >= N) break;
        const int k = clamp_code(idx[row], K);
        const float* e = cb + (long)k * D;
        const float* zp = z + (long)row * ldz;
        for (int j = lane; j < D; j += 64) {
            const float ev = e[j];
            const float d = ev - zp[j];
            acc += (double)d * (double)d;
            zq[(long)row * ldo + j] = ev;
        }
        if (img != nullptr) {
            if constexpr (H2IMG) {
                for (int g = lane; g < (n_store >> 3); g += 64) {
                    float v[8];
#pragma unroll
                    for (int c = 0; c < 8; ++c) v[c] = 8 * g + c < D ? e[8 * g + c] : 0.f;
                    emage_dev::h2_store8((emage_dev::h2_t*)img + (long)row * ld_img + 8 * g, v, h2s);
                }
            } else {
                for (int j = lane; j < n_store; j += 64) img[(long)row * ld_img + j] = Elem<T>::to(j < D ? e[j] : 0.f);
            }
        }
        if (lane == 0) atomicAdd(&hist[k], 1);
    }
    acc = wave_sum(acc);
    if (lane == 0) s_part[wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.x] = ((s_part[0] + s_part[1]) + s_part[2]) + s_part[3];
}

// One block: scalars[0] = (1 + beta) * sum(partials) / (N D), scalars[1] = exp(-sum_k p_k log(p_k + 1e-10)), p = hist / N.
__global__ __launch_bounds__(256) void vq_quantize_finalize(const double* __restrict__ partials, int n_partials, const int* __restrict__ hist,
                                                            float* __restrict__ scalars, float beta, int N, int K, int D) {
    __shared__ double s_a[4], s_b[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double a = 0.0, b = 0.0;
    for (int i = threadIdx.x; i < n_partials; i += 256) a += partials[i];
    for (int k = threadIdx.x; k < K; k += 256) {
        const double p = (double)hist[k] / (double)N;
        b += p * log(p + 1e-10);
    }
    a = wave_sum(a);
    b = wave_sum(b);
    if (lane == 0) { s_a[wave] = a; s_b[wave] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const double mse = (((s_a[0] + s_a[1]) + s_a[2]) + s_a[3]) / ((double)N * (double)D);
        scalars[0] = (float)(mse + (double)beta * mse);
        scalars[1] = (float)exp(-(((s_b[0] + s_b[1]) + s_b[2]) + s_b[3]));
    }
}

// dz[n] = g_zq[n] + g_loss * beta * (2 / (N D)) * (z[n] - e[idx[n]]): one block per row.
__global__ __launch_bounds__(256) void vq_quantize_backward_dz(const float* __restrict__ z, int ldz, const float* __restrict__ cb,
                                                               const int64_t* __restrict__ idx, const float* __restrict__ g_zq, int ldg,
                                                               const float* __restrict__ g_loss, float beta, float* __restrict__ dz, int ld_dz,
                                                               int N, int K, int D) {
    const int row = blockIdx.x;
    const float coef = (float)((double)g_loss[0] * (double)beta * 2.0 / ((double)N * (double)D));
    const float* e = cb + (long)clamp_code(idx[row], K) * D;
    for (int j = threadIdx.x; j < D; j += 256) {
        const float c = coef * (z[(long)row * ldz + j] - e[j]);
        dz[(long)row * ld_dz + j] = g_zq != nullptr ? g_zq[(long)row * ldg + j] + c : c;
    }
}

// dE[k] = g_loss * (2 / (N D)) * sum_{n : idx[n] = k} (e[k] - z[n]): one block per code.  Every wave reads the index list 64 entries at
// a time (coalesced; the whole list sits in L2), forms the match mask with a ballot and walks its set bits from the lowest up, so the rows
// of a code are added in ascending n — a fixed order, in float64.  Thread t owns columns t, t + 256, ... (D <= 1024).
__global__ __launch_bounds__(256) void vq_quantize_backward_de(const float* __restrict__ z, int ldz, const float* __restrict__ cb,
                                                               const int64_t* __restrict__ idx, const float* __restrict__ g_loss,
                                                               float* __restrict__ dE, int N, int K, int D) {
    const int k = blockIdx.x, lane = threadIdx.x & 63;
    float ev[4];
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int j = threadIdx.x + 256 * c;
        ev[c] = j < D ? cb[(long)k * D + j] : 0.f;
    }
    for (int n0 = 0; n0 < N; n0 += 64) {
        const int n = n0 + lane;
        const bool hit = n < N && idx[n] == (int64_t)k;
        unsigned long long mask = __ballot(hit);
        while (mask) {
            const int b = __ffsll((long long)mask) - 1;
            mask &= mask - 1;
            const float* zp = z + (long)(n0 + b) * ldz;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                const int j = threadIdx.x + 256 * c;
                if (j < D) acc[c] += (double)(ev[c] - zp[j]);
            }
        }
    }
    const double coef = (double)g_loss[0] * 2.0 / ((double)N * (double)D);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int j = threadIdx.x + 256 * c;
        if (j < D) dE[(long)k * D + j] = (float)(coef * acc[c]);
    }
}

}  // namespace

extern "C" long emage_vq_quantize_train_workspace_bytes(int N) {
    return N <= 0 ? 0 : (long)((N + QT_ROWS - 1) / QT_ROWS) * (long)sizeof(double);
}

extern "C" int emage_vq_quantize_train(const float* z, int ldz, const float* codebook, const int64_t* idx, float* zq, int ldo,
                                       void* zq_image, int ld_image, int n_store, int dtype, int* hist, float* scalars, float beta,
                                       void* workspace, long workspace_bytes, int N, int K, int D, void* stream) {
    if (!z || !codebook || !idx || !zq || !hist || !scalars || !workspace || N <= 0 || K <= 0 || K > 4096 || D <= 0 || D > 1024 || ldz < D || ldo < D)
        return EMAGE_EINVAL;
    if (workspace_bytes < emage_vq_quantize_train_workspace_bytes(N) || ((uintptr_t)workspace & 7)) return EMAGE_EINVAL;
    emage_dev::H2Scale hs;
    if (emage_dev::h2_dtype(dtype, hs)) return EMAGE_EINVAL;
    if (zq_image) {
        if (n_store < D || ld_image < n_store) return EMAGE_EINVAL;
        if (dtype != EMAGE_F32 && dtype != EMAGE_BF16 && dtype != EMAGE_H2) return EMAGE_EINVAL;
        if (dtype == EMAGE_H2 && (n_store % 8 || ld_image % 8 || ((uintptr_t)zq_image & 15))) return EMAGE_EINVAL;
    }
    hipStream_t s = (hipStream_t)stream;
    const int blocks = (N + QT_ROWS - 1) / QT_ROWS;
    hipError_t e = hipMemsetAsync(hist, 0, (size_t)K * sizeof(int), s);
    if (e != hipSuccess) return (int)e;
    double* partials = (double*)workspace;
    if (zq_image && dtype == EMAGE_H2)
        hipLaunchKernelGGL((vq_quantize_train<float, true>), dim3(blocks), dim3(256), 0, s, z, ldz, codebook, idx, zq, ldo, (float*)zq_image, ld_image, n_store,
                           hs.s, hist, partials, N, K, D);
    else if (zq_image && dtype == EMAGE_BF16)
        hipLaunchKernelGGL((vq_quantize_train<bf16_t, false>), dim3(blocks), dim3(256), 0, s, z, ldz, codebook, idx, zq, ldo, (bf16_t*)zq_image, ld_image, n_store,
                           1.f, hist, partials, N, K, D);
    else
        hipLaunchKernelGGL((vq_quantize_train<float, false>), dim3(blocks), dim3(256), 0, s, z, ldz, codebook, idx, zq, ldo, (float*)zq_image, ld_image, n_store,
                           1.f, hist, partials, N, K, D);
    hipLaunchKernelGGL(vq_quantize_finalize, dim3(1), dim3(256), 0, s, partials, blocks, hist, scalars, beta, N, K, D);
    return launch_status();
}

extern "C" int emage_vq_quantize_backward(const float* z, int ldz, const float* codebook, const int64_t* idx, const float* g_zq, int ldg,
                                          const float* g_loss, float beta, float* dz, int ld_dz, float* d_codebook, int N, int K, int D,
                                          void* stream) {
    if (!z || !codebook || !idx || !g_loss || !dz || !d_codebook || N <= 0 || K <= 0 || K > 4096 || D <= 0 || D > 1024 || ldz < D || ld_dz < D)
        return EMAGE_EINVAL;
    if (g_zq && ldg < D) return EMAGE_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(vq_quantize_backward_dz, dim3(N), dim3(256), 0, s, z, ldz, codebook, idx, g_zq, ldg, g_loss, beta, dz, ld_dz, N, K, D);
    hipLaunchKernelGGL(vq_quantize_backward_de, dim3(K), dim3(256), 0, s, z, ldz, codebook, idx, g_loss, d_codebook, N, K, D);
    return launch_status();
}
