// Host plumbing of a fused attention site (qkv_attention.hip, q_attention.hip): a projection run by gemm_h2_tile whose epilogue feeds attn_tile
// in the same launch, one workgroup per (clip, head), up to G sites per grid.  A site is its kernel and its `make_problem` (what it takes
// beside the projection's operands, and the limits of that); the argument block, the refusals every site shares, the projection's GemmArgs
// and the launch are here.
#pragma once
#include "common.h"
#include "gemm_tile.h"
#include "h2.h"

namespace emage_dev {

// the argument block of one launch, by value (kernarg segment): the sites' arguments and the running sum of their blocks (B H); the unused
// entries repeat p[0].  A block finds its site with site_block.
template <class P, int G> struct SiteGroup {
    static constexpr int MAXG = G;
    P p[G];
    int blk_end[G];
    int n, total;
};

// This block's site in the group, and its clip b and head h (of H) there.  XCD-aware order over the whole grid (gemm_h2.hip:
// gemm_h2_group_kernel): each XCD walks a contiguous run of (clip, head) blocks, heads fastest — the heads of a clip share A.
template <int H, class P, int G> __device__ __forceinline__ const P& site_block(const SiteGroup<P, G>& g, int& b, int& h) {
    const int bid = xcd_run_order((int)blockIdx.x, g.total);
    int pi = 0;
#pragma unroll
    for (int i = 0; i < G - 1; ++i) pi += (i + 1 < g.n && bid >= g.blk_end[i]) ? 1 : 0;
    pi = __builtin_amdgcn_readfirstlane(pi);
    const int t = bid - (pi ? g.blk_end[pi - 1] : 0);
    b = t / H;
    h = t - b * H;
    return g.p[pi];
}

// What a site's epilogue stages for one accumulator: emage_gemm's float32 value of that column, operation for operation (no contraction of
// a * b + c in this build), from operands the kernel has already loaded.  The projection's value in front of its bias: o_scale, then the
// folded LayerNorm (fold: wave-uniform) ...
__device__ __forceinline__ float site_x(const float acc, const float os, const bool fold, const float rs, const float mu, const float c) {
    float x = acc * os;
    if (fold) x = rs * (x - mu * c);
    return x;
}
// ... as the row-major epilogue ends it (h2_tile_epilogue with no slope and no residual: leaky(., 1), + 0) — q, k
__device__ __forceinline__ float site_row_value(const float x, const float bias) {
    float y = x + bias;
    y = leaky(y, 1.f);
    y += 0.f;
    return y;
}
// ... and as the V^T epilogue does — v
__device__ __forceinline__ float site_vt_value(const float x, const float bias) { return leaky(x + bias, 1.f); }

// The refusals every site shares, on the fields every site's problem struct carries (A, W, bias, out, lda, ldo, B, the scales, the LayerNorm
// fold): EMAGE_H2 only (`dtype` after h2_dtype), operands present and 16-byte aligned, row pitches that hold d columns in whole h2 groups,
// positive scales, a complete fold, byte offsets below 2^31.
template <class Q> int site_check(int dtype, const Q& q, int T, int d) {
    if (dtype != EMAGE_H2) return EMAGE_EINVAL;
    if (!q.A || !q.W || !q.bias || !q.out || q.B <= 0) return EMAGE_EINVAL;
    if (((uintptr_t)q.A | (uintptr_t)q.W | (uintptr_t)q.bias | (uintptr_t)q.out) & 15) return EMAGE_EINVAL;
    if (q.lda % 8 || q.lda < d || q.ldo % 8 || q.ldo < d) return EMAGE_EINVAL;
    if (!(q.a_scale > 0.f && q.w_scale > 0.f)) return EMAGE_EINVAL;
    if (q.ln_stats && (!q.ln_c || ((uintptr_t)q.ln_stats & 15) || ((uintptr_t)q.ln_c & 15) || !(q.ln_eps > 0.f))) return EMAGE_EINVAL;
    const long rows = (long)q.B * T;
    if (rows * q.lda * 4 >= (1L << 31) || rows * q.ldo * 4 >= (1L << 31)) return EMAGE_EINVAL;
    return 0;
}

// the site's projection as emage_gemm runs it: (B T, d) x (N, d)^T, no outputs of its own (the V^T column range starts behind the last column)
template <class Q> GemmArgs site_projection(const Q& q, int T, int N, int d, const H2Scale& hs) {
    GemmArgs a = {};
    a.A = q.A; a.W = q.W; a.bias = q.bias;
    a.lda = q.lda;
    a.M = q.B * T; a.N = N; a.K = d; a.Cp = d;
    set_geometry(a, 1, 1, 0, a.M, a.M);
    a.t_col0 = a.N; a.t_rows = 1;
    a.ksplit = 1;
    a.a_scale = q.a_scale;
    a.o_scale = 1.f / (q.a_scale * q.w_scale);    // as emage_gemm computes it
    a.h2s = hs.s; a.h2i = hs.inv;
    a.ln_stats = q.ln_stats; a.ln_np = q.ln_stats ? 24 : 0; a.ln_c = q.ln_stats ? q.ln_c : nullptr; a.ln_eps = q.ln_eps;
    return a;
}

// problems[0..n) -> one launch of `kernel` (taking the group `Group` by value) with `heads` blocks per clip; make(dtype, problem, hs, args)
// is the site's make_problem
template <class Group, class Q, class Make>
int launch_sites(int dtype, const Q* problems, int n, int heads, Make make, void (*kernel)(Group), int threads, hipStream_t s) {
    H2Scale hs;
    if (h2_dtype(dtype, hs) || !problems || n <= 0 || n > Group::MAXG) return EMAGE_EINVAL;
    Group g;
    int total = 0;
    for (int i = 0; i < n; ++i) {
        const int rc = make(dtype, problems[i], hs, g.p[i]);
        if (rc) return rc;
        total += problems[i].B * heads;
        g.blk_end[i] = total;
    }
    for (int i = n; i < Group::MAXG; ++i) { g.p[i] = g.p[0]; g.blk_end[i] = total; }
    g.n = n;
    g.total = total;
    hipLaunchKernelGGL(kernel, dim3(total), dim3(threads), 0, s, g);
    return launch_status();
}

}  // namespace emage_dev
