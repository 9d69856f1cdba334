// The gradient of an embedding table that is read ONE ROW PER CLIP (EmageAudioModel's speaker_embedding_body / _face, M:217-219, 285-286:
// `gather_rows(table, ids broadcast over T)`):
//   dw[s][c] = sum over clips b with clamp(ids[b]) == s, b ascending, of sum over t < T, t ascending, of g[(b * T + t) * ldg + c]
// in float64, rounded to fp32 once; no atomics, so the same inputs give the same bits in every run and every graph replay (the convention of
// vq_quantize_backward_de and col_reduce.h).  Two launches, so that no workgroup walks all B * T rows of a speaker:
//   embedding_clip_sums   grid (clip, 256-column block): thread c adds its column of the clip's T rows into ws[b * D + c] (float64)
//   embedding_row_sums    grid (table row, 256-column block): thread c walks the id list (B entries, the same address in every lane: one
//                         broadcast read each) and adds ws[b * D + c] of the matching clips in ascending b; a row no clip names is written 0.0f
// The clamp is gather_rows' (csrc/vq.hip): below 0 -> 0, at or above S -> S - 1; nothing is ever indexed with an unclamped id.
#include "common.h"

namespace {

constexpr int THREADS = 256;

__global__ __launch_bounds__(THREADS) void embedding_clip_sums(const float* __restrict__ g, long ldg, int T, int D, double* __restrict__ ws) {
    const int c = blockIdx.y * THREADS + threadIdx.x;
    if (c >= D) return;
    const long b = blockIdx.x;
    const float* gp = g + b * T * ldg + c;
    double acc = 0.0;
    int t = 0;
    for (; t + 8 <= T; t += 8) {                         // eight independent loads in flight, added in ascending t
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = gp[(long)(t + i) * ldg];
#pragma unroll
        for (int i = 0; i < 8; ++i) acc += (double)v[i];
    }
    for (; t < T; ++t) acc += (double)gp[(long)t * ldg];
    ws[b * D + c] = acc;
}

__global__ __launch_bounds__(THREADS) void embedding_row_sums(const double* __restrict__ ws, const int64_t* __restrict__ ids, int B, int D, int S,
                                                              float* __restrict__ dw, long lddw) {
    const int c = blockIdx.y * THREADS + threadIdx.x;
    if (c >= D) return;
    const long s = blockIdx.x;
    double acc = 0.0;
    for (long b = 0; b < B; ++b) {
        long k = ids[b];
        k = k < 0 ? 0 : (k >= S ? S - 1 : k);
        if (k == s) acc += ws[b * D + c];
    }
    dw[s * lddw + c] = (float)acc;
}

}  // namespace

extern "C" long emage_embedding_backward_workspace_bytes(int B, int D) {
    return (B <= 0 || D <= 0) ? 0 : (long)B * (long)D * (long)sizeof(double);
}

extern "C" int emage_embedding_backward(const float* g, long ldg, const int64_t* ids, int B, int T, int D, int S, float* dw, long lddw,
                                        void* workspace, long workspace_bytes, void* stream) {
    if (!g || !ids || !dw || !workspace || B <= 0 || T <= 0 || D <= 0 || D > 4096 || S <= 0 || S > 1024 || ldg < D || lddw < D) return EMAGE_EINVAL;
    if (workspace_bytes < emage_embedding_backward_workspace_bytes(B, D) || ((uintptr_t)workspace & 7)) return EMAGE_EINVAL;
    hipStream_t s = (hipStream_t)stream;
    const unsigned col_blocks = (unsigned)((D + THREADS - 1) / THREADS);
    hipLaunchKernelGGL(embedding_clip_sums, dim3((unsigned)B, col_blocks), dim3(THREADS), 0, s, g, ldg, T, D, (double*)workspace);
    hipLaunchKernelGGL(embedding_row_sums, dim3((unsigned)S, col_blocks), dim3(THREADS), 0, s, (const double*)workspace, ids, B, D, S, dw, lddw);
    return launch_status();
}
