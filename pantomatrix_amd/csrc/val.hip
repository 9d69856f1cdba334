// The metrics of one validation step (train_emage_audio.py:130-204 with mode="val": three eval forwards, get_rec_loss / get_cls_loss of each,
// the arg-max codes of the first) in TWO launches instead of 24 loss launches and 4 arg-max launches, over the REAL clips of a padded batch:
//   val_rows_kernel      grid (row blocks, entries).  One wave per row, ROWS_PER_WAVE rows per wave.  Per row of an entry (one forward x one
//                        body part): the (M, K) logits row is staged in LDS with 16-byte loads and walked by `row_logsoftmax_argmax`
//                        (argmax_row.h: the arithmetic of emage_argmax_logsoftmax_f32, so the same index), NLL at index_gt, hit = (arg-max ==
//                        index_gt); the (M, C) latent rows are read with 16-byte loads, difference and square in fp32, sum in float64.  Rows
//                        at or beyond n_valid * T (n_valid: one int32 in device memory) only write their pred_index.  Each block stores ONE
//                        partial {mse, nll, hits, bad index seen} into the workspace: no atomics, a fixed summation order.
//   val_finalize_kernel  one block.  Wave w folds the partials of entries w, w + 4, w + 8 in block order; thread 0 turns the sums into the
//                        reference's per-batch values, writes last[7], adds to meter[7], the hit / row / batch counters and the status word.
// Bound: memory.  A row is K * 4 bytes of logits + 2 * C * 4 bytes of latents (3 KB at K = C = 256), read once; the arithmetic is ~3 K flops
// and K expf per row.  56 x 64 rows x 12 entries = 129 MB per validation step: ~20 us at HBM rate, in practice the launch and the tail.
#include "common.h"
#include "argmax_row.h"

namespace {

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int ROWS_PER_WAVE = 4, ROWS_PER_BLOCK = WAVES * ROWS_PER_WAVE;
constexpr int MAX_WIDTH = EMAGE_VAL_MAX_WIDTH;

struct Partial { double mse, nll; long long hits, bad; };                 // 32 bytes: one per (entry, row block)
struct Table { emage_val_entry e[EMAGE_VAL_MAX_ENTRIES]; };               // by value in the kernel arguments: nothing a captured graph must keep alive

__device__ __forceinline__ int real_rows(const int* n_valid, int M, int T) {
    int n = *n_valid;
    const int clips = M / T;
    n = n < 0 ? 0 : (n > clips ? clips : n);
    return n * T;
}

__device__ __forceinline__ bool aligned16(const float* p, int ld) { return (((uintptr_t)p & 15) == 0) && (ld % 4 == 0); }

__global__ __launch_bounds__(THREADS) void val_rows_kernel(Table tab, int M, int T, const int* __restrict__ n_valid, Partial* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float s_x[WAVES][MAX_WIDTH];
    __shared__ Partial s_p[WAVES];
    const emage_val_entry& en = tab.e[blockIdx.y];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int rows = real_rows(n_valid, M, T);
    const int K = en.K, C = en.C;
    const bool vec_x = aligned16(en.logits, en.ld_logits), vec_r = aligned16(en.rec, en.ld_rec) && aligned16(en.latent, en.ld_latent);
    const IdxView iv{en.pred_rows, en.pred_ld, 1};
    double mse = 0.0, nll = 0.0;
    long long hits = 0, bad = 0;
    for (int i = 0; i < ROWS_PER_WAVE; ++i) {
        const int row = blockIdx.x * ROWS_PER_BLOCK + i * WAVES + wave;            // wave-uniform
        if (row >= M) break;
        const bool real = row < rows;
        if (!real && !en.pred) continue;
        // the logits row -> LDS (16-byte loads when the view allows them), then the classifier row of emage_argmax_logsoftmax_f32 over it
        const float* xp = en.logits + (long)row * en.ld_logits;
        float* sx = s_x[wave];
        const int k4 = vec_x ? (K & ~3) : 0;
        for (int c = 4 * lane; c < k4; c += 256) *(float4*)(sx + c) = *(const float4*)(xp + c);
        for (int c = k4 + lane; c < K; c += 64) sx[c] = xp[c];
        __builtin_amdgcn_wave_barrier();
        float mx, ls, bd; int bi;
        row_logsoftmax_argmax([&](int c) { return sx[c]; }, K, lane, mx, ls, bd, bi);
        if (en.pred && lane == 0) en.pred[idx_at(iv, row)] = (int64_t)bi;
        if (real) {
            const int64_t t = en.index[row];
            if (t < 0 || t >= K) bad = 1;
            else {
                nll += (double)(-__fsub_rn(__fsub_rn(sx[t], mx), ls));
                hits += (bi == (int)t) ? 1 : 0;
            }
            // sum_c (rec - latent)^2: difference and square in fp32 (torch's mse_loss), the sum in float64
            const float* rp = en.rec + (long)row * en.ld_rec;
            const float* gp = en.latent + (long)row * en.ld_latent;
            double s = 0.0;
            const int c4 = vec_r ? (C & ~3) : 0;
            for (int c = 4 * lane; c < c4; c += 256) {
                const float4 a = *(const float4*)(rp + c), b = *(const float4*)(gp + c);
                const float d0 = a.x - b.x, d1 = a.y - b.y, d2 = a.z - b.z, d3 = a.w - b.w;
                s += (double)(d0 * d0);
                s += (double)(d1 * d1);
                s += (double)(d2 * d2);
                s += (double)(d3 * d3);
            }
            for (int c = c4 + lane; c < C; c += 64) {
                const float d = rp[c] - gp[c];
                s += (double)(d * d);
            }
            for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m);
            mse += s;
        }
        __builtin_amdgcn_wave_barrier();                                           // the next row overwrites this wave's LDS row
    }
    if (lane == 0) s_p[wave] = Partial{mse, nll, hits, bad};
    __syncthreads();
    if (threadIdx.x == 0) {
        Partial p = s_p[0];
        for (int w = 1; w < WAVES; ++w) { p.mse += s_p[w].mse; p.nll += s_p[w].nll; p.hits += s_p[w].hits; p.bad |= s_p[w].bad; }
        partial[(long)blockIdx.y * gridDim.x + blockIdx.x] = p;
    }
}

__global__ __launch_bounds__(THREADS) void val_finalize_kernel(Table tab, int n_entries, int blocks, int M, int T, const int* __restrict__ n_valid,
                                                               const Partial* __restrict__ partial, double* __restrict__ acc) {
    __shared__ Partial s_e[EMAGE_VAL_MAX_ENTRIES];
    const int rows = real_rows(n_valid, M, T);
    if (rows == 0) return;                                                        // an empty batch changes nothing (uniform: no barrier is skipped by a part of the block)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int e = wave; e < n_entries; e += WAVES) {
        Partial p{0.0, 0.0, 0, 0};
        for (int b = lane; b < blocks; b += 64) {
            const Partial q = partial[(long)e * blocks + b];
            p.mse += q.mse; p.nll += q.nll; p.hits += q.hits; p.bad |= q.bad;
        }
        for (int m = 32; m >= 1; m >>= 1) {
            p.mse += __shfl_xor(p.mse, m); p.nll += __shfl_xor(p.nll, m); p.hits += __shfl_xor(p.hits, m); p.bad |= __shfl_xor(p.bad, m);
        }
        if (lane == 0) s_e[e] = p;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double last[EMAGE_VAL_LOSSES] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    long long* counters = (long long*)acc;
    long long bad = 0;
    for (int e = 0; e < n_entries; ++e) {                                          // table order: a fixed order of the float64 adds
        const emage_val_entry& en = tab.e[e];
        last[2 * en.tag] += en.l_w * (s_e[e].mse / ((double)rows * en.C));
        last[2 * en.tag + 1] += en.c_w * (s_e[e].nll / (double)rows);
        counters[EMAGE_VAL_ACC_HITS + e] += s_e[e].hits;
        counters[EMAGE_VAL_ACC_LAST_HITS + e] = s_e[e].hits;
        bad |= s_e[e].bad;
    }
    for (int k = 0; k < EMAGE_VAL_LOSSES - 1; ++k) last[EMAGE_VAL_LOSSES - 1] += last[k];
    for (int k = 0; k < EMAGE_VAL_LOSSES; ++k) {
        acc[EMAGE_VAL_ACC_LAST + k] = last[k];
        acc[EMAGE_VAL_ACC_METER + k] += last[k];
    }
    counters[EMAGE_VAL_ACC_ROWS] += rows;
    counters[EMAGE_VAL_ACC_LAST_ROWS] = rows;
    counters[EMAGE_VAL_ACC_BATCHES] += 1;
    if (bad) counters[EMAGE_VAL_ACC_STATUS] |= 1;
}

int row_blocks(int M) { return (M + ROWS_PER_BLOCK - 1) / ROWS_PER_BLOCK; }

}  // namespace

extern "C" long emage_val_metrics_workspace_bytes(int M, int n_entries) {
    if (M <= 0 || n_entries <= 0 || n_entries > EMAGE_VAL_MAX_ENTRIES) return EMAGE_EINVAL;
    return (long)row_blocks(M) * n_entries * (long)sizeof(Partial);
}

extern "C" int emage_val_metrics(const emage_val_entry* entries, int n_entries, int M, int T, const int* n_valid, void* acc,
                                 void* workspace, long workspace_bytes, void* stream) {
    if (!entries || !n_valid || !acc || !workspace || n_entries <= 0 || n_entries > EMAGE_VAL_MAX_ENTRIES) return EMAGE_EINVAL;
    if (M <= 0 || T <= 0 || M % T != 0) return EMAGE_EINVAL;
    if (((uintptr_t)acc & 7) || ((uintptr_t)workspace & 7) || ((uintptr_t)n_valid & 3)) return EMAGE_EINVAL;
    if (workspace_bytes < emage_val_metrics_workspace_bytes(M, n_entries)) return EMAGE_EINVAL;
    Table tab{};
    for (int i = 0; i < n_entries; ++i) {
        const emage_val_entry& e = entries[i];
        if (!e.rec || !e.latent || !e.logits || !e.index) return EMAGE_EINVAL;
        if (e.K < 2 || e.K > MAX_WIDTH || e.C < 1 || e.C > MAX_WIDTH) return EMAGE_EINVAL;
        if (e.ld_rec < e.C || e.ld_latent < e.C || e.ld_logits < e.K) return EMAGE_EINVAL;
        if (e.tag < 0 || e.tag >= EMAGE_VAL_TAGS || !(e.l_w == e.l_w) || !(e.c_w == e.c_w)) return EMAGE_EINVAL;
        if (e.pred && e.pred_rows > 0 && (M % e.pred_rows != 0 || e.pred_ld < e.pred_rows)) return EMAGE_EINVAL;
        if (((uintptr_t)e.rec | (uintptr_t)e.latent | (uintptr_t)e.logits) & 3 || ((uintptr_t)e.index | (uintptr_t)e.pred) & 7) return EMAGE_EINVAL;
        tab.e[i] = e;
    }
    const int blocks = row_blocks(M);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(val_rows_kernel, dim3(blocks, n_entries), dim3(THREADS), 0, s, tab, M, T, n_valid, (Partial*)workspace);
    int rc = launch_status();
    if (rc) return rc;
    hipLaunchKernelGGL(val_finalize_kernel, dim3(1), dim3(THREADS), 0, s, tab, n_entries, blocks, M, T, n_valid, (const Partial*)workspace, (double*)acc);
    return launch_status();
}
