// The deterministic float64 reductions of the training kernels (train.hip, train_backward.hip, optim.hip): chunked column sums
// (partials per chunk of rows, then a finalize over the chunks), the LDS halving tree of a block, the shuffle sum of a wave, and the
// host-side grid helpers that go with them.  No atomics anywhere: the same input gives the same bits.
#pragma once
#include "common.h"

constexpr int STAT_ROWS = 4;          // row lanes per block: 4 x 64 columns = 256 threads
constexpr int STAT_CHUNK = 64;        // least rows per block (2048 left the small-M layers of a training step with ~24 blocks on 256 CUs: 130 us per
                                      // bias gradient, 17 % of the step — profiles/r03_train_kernel_stats_before.csv)

// rows per partial block: STAT_CHUNK at least, at most ~512 chunks (the finalize kernels add the chunks of a column in a fixed order: deterministic)
static inline int stat_rows(int M) {
    int r = ((M + 511) / 512 + 3) & ~3;
    return r < STAT_CHUNK ? STAT_CHUNK : r;
}

// The partial step of a chunked column reduction of NV values per column; grid (chunks, ceil(C / 64)), 256 threads = STAT_ROWS row lanes x 64
// columns.  Block (k, j) takes rows [k * chunk_rows, (k + 1) * chunk_rows) of columns 64 j .. 64 j + 63: row lane l adds rows l, l + 4, ... of its
// column through row_term(r, c, s) (s[v] += row r's contribution), lane 0 adds the four lane sums in order and writes
// partial[(chunk * NV + v) * C + c].  stat_column() is the column of the calling thread, for per-column constants set up in front.
__device__ __forceinline__ int stat_column() { return blockIdx.y * 64 + (threadIdx.x & 63); }
template <int NV, typename RowTerm>
__device__ __forceinline__ void column_partials(int M, int C, int chunk_rows, double* __restrict__ partial, RowTerm row_term) {
    __shared__ double red[NV][STAT_ROWS][64];
    const int cl = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = stat_column();
    const long r0 = (long)blockIdx.x * chunk_rows;
    const long r1 = r0 + chunk_rows < M ? r0 + chunk_rows : M;
    double s[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) s[v] = 0.0;
    if (c < C)
        for (long r = r0 + rl; r < r1; r += STAT_ROWS) row_term(r, c, s);
#pragma unroll
    for (int v = 0; v < NV; ++v) red[v][rl][cl] = s[v];
    __syncthreads();
    if (rl == 0 && c < C) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            double a = 0.0;
            for (int i = 0; i < STAT_ROWS; ++i) a += red[v][i][cl];
            partial[((long)blockIdx.x * NV + v) * C + c] = a;
        }
    }
}

// The finalize step of every chunked column reduction: 16 columns x 16 lanes per block; lane l adds its contiguous range of
// chunks in order, lane 0 then adds the 16 lane sums in order — deterministic for a given chunk count, and 16x shorter than one thread
// walking all (up to 512) chunks of its column (which cost 20-80 us per call: 14 % of a training step,
// profiles/r03_train_kernel_stats_final.csv).  partial[(chunk * NV + v) * C + c]; `block` is the block's index WITHIN this reduction
// (blockIdx.x when the launch holds one reduction); true for the thread that holds column c_out's totals.
constexpr int FIN_COLS = 16, FIN_LANES = 16;
constexpr int FIN_THREADS = FIN_COLS * FIN_LANES;
template <int NV>
__device__ __forceinline__ bool finalize_sums(const double* __restrict__ partial, int chunks, int C, int block, double (&tot)[NV], int& c_out) {
    __shared__ double red[NV][FIN_LANES][FIN_COLS];
    const int cl = threadIdx.x % FIN_COLS, rl = threadIdx.x / FIN_COLS;
    const int c = block * FIN_COLS + cl;
    const int per = (chunks + FIN_LANES - 1) / FIN_LANES;
    const int i0 = rl * per, i1 = i0 + per < chunks ? i0 + per : chunks;
    double s[NV];
#pragma unroll
    for (int v = 0; v < NV; ++v) s[v] = 0.0;
    if (c < C)
        for (int i = i0; i < i1; ++i)
#pragma unroll
            for (int v = 0; v < NV; ++v) s[v] += partial[((long)i * NV + v) * C + c];
#pragma unroll
    for (int v = 0; v < NV; ++v) red[v][rl][cl] = s[v];
    __syncthreads();
    c_out = c;
    if (rl != 0 || c >= C) return false;
#pragma unroll
    for (int v = 0; v < NV; ++v) {
        double a = 0.0;
        for (int l = 0; l < FIN_LANES; ++l) a += red[v][l][cl];
        tot[v] = a;
    }
    return true;
}
static inline int fin_blocks(int C) { return (C + FIN_COLS - 1) / FIN_COLS; }
static inline dim3 fin_grid(int C) { return dim3(fin_blocks(C)); }

// The sum of red[0 .. THREADS) (one value per thread of the block, written by the caller) by a halving tree in LDS; every thread gets it.
template <int THREADS>
__device__ __forceinline__ double block_tree_sum(double* red) {
    __syncthreads();
    for (int w = THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ double wave_sum(double s) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    return s;                                             // lane 0 holds the sum
}

// grid of a grid-stride elementwise kernel of 256 threads
static inline int grid_for(long total) {
    long g = (total + 255) / 256;
    return (int)(g > 8192 ? 8192 : (g < 1 ? 1 : g));
}

// grid of a loss partial kernel: one float64 partial per block in the loss workspace, whose last slot is the nll `bad` flag
constexpr int LOSS_BLOCKS = EMAGE_LOSS_WORKSPACE_BYTES / 8;
static inline int loss_grid(long total) {
    long g = (total + 255) / 256;
    return (int)(g > LOSS_BLOCKS - 1 ? LOSS_BLOCKS - 1 : (g < 1 ? 1 : g));
}
