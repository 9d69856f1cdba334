// emage_qkv_attention — one self-attention site of the EMAGE transformer layers (T = 64 frames, d = 768, 4 heads of 192) as ONE launch
// instead of the qkv projection (emage_gemm, config 100 / 1100: q / k float32 and V^T float32 to memory) followed by emage_attention
// (which reads them back).  One workgroup per (clip, head): at T = 64 the projection's row tile IS one clip, and everything the attention
// of head h needs are the 3 x 192 output columns q_h, k_h, v_h of those 64 rows.
//   * K-loop: gemm_h2_tile (h2_tile.h) unchanged on a 64 x 576 block tile — the 576 W rows are the three 192-row slices of head h
//     (SEGS = 3) — 8 waves of 16 x 288 (WTM = 16 as in config 100, so the folded LayerNorm's statistics merge in the same order);
//   * epilogue: the arithmetic of h2_tile_epilogue for these columns (o_scale, the LayerNorm fold, bias; q / k as the row-major float32
//     path computes them, v as the V^T path does: attn_site.h), then split into fp16 planes straight into the operand ring, in the layout
//     attn_stage_kv gives K / V^T (and K's layout for Q) — AttnLds in attn_tile.h, through its attn_store_row8 / attn_store_vt8;
//   * attention: attn_tile on LDS fragments (QLDS), four waves of 16 queries; `att` is written as the EMAGE_H2 image.
// Every q / k / v value, every split plane and the order of every MFMA over its contraction are those of the two-launch sequence: the
// output is the same bits (tests/test_qkv_attention_gpu.py).
#include "common.h"
#include <math.h>
#include "h2_tile.h"
#include "attn_tile.h"
#include "attn_site.h"

namespace emage_dev {

constexpr int QA_T = 64, QA_HD = 192, QA_H = 4, QA_D = QA_H * QA_HD;
constexpr int QA_BM = 64, QA_BN = 3 * QA_HD, QA_WM = 4, QA_WN = 2, QA_NS = 2;
constexpr int QA_THREADS = QA_WM * QA_WN * 64;
constexpr int QA_MAXG = 4;

struct QkvAttnArgs {
    GemmArgs g;              // the projection as emage_gemm runs it (M = B T, N = 3 d, K = d; no outputs of its own)
    void* out; int ldo;      // att: (B T, ldo) EMAGE_H2 image
};
using QkvAttnGroup = SiteGroup<QkvAttnArgs, QA_MAXG>;

}  // namespace emage_dev

namespace {

using namespace emage_dev;
using L = AttnLds<QA_HD, 4>;
static_assert(L::BYTES + L::K_BYTES <= h2_smem_bytes<QA_BM, QA_BN, QA_NS>(), "K, V^T and Q fit the operand ring");
static_assert(h2_smem_bytes<QA_BM, QA_BN, QA_NS>() <= 160 * 1024, "one block per CU");

__global__ __launch_bounds__(QA_THREADS, 1) void qkv_attn_kernel(QkvAttnGroup g) {
    __shared__ __attribute__((aligned(128))) unsigned char smem[h2_smem_bytes<QA_BM, QA_BN, QA_NS>()];
    int b, h;
    const QkvAttnArgs& q = site_block<QA_H>(g, b, h);
    const GemmArgs& p = q.g;

    // the epilogue: q / k / v of this wave's 16 frames x 288 columns -> split planes in LDS
    auto epi = [&](auto& acc, const int, const int wm, const int wn, const int fr, const int fg, const auto& ln_mu, const auto& ln_rs) {
        __syncthreads();                               // every wave has read its last fragments of the ring
        const float os = p.o_scale;
        const int fm = wm * 16 + fr;                   // frame of this lane's row
        static_for<QA_BN / 2 / 32>([&](auto jc) {
            constexpr int JP = decltype(jc)::value;
            const int c = wn * (QA_BN / 2) + JP * 32;           // first column of the fragment pair in the block tile (wave-uniform)
            const int seg = c >= 2 * QA_HD ? 2 : c >= QA_HD ? 1 : 0;      // q / k / v
            const int cc = c - seg * QA_HD + fg * 8;            // this lane's 8 columns inside the head: cc .. cc + 7
            const int n = seg * (p.N / 3) + h * QA_HD + cc;     // ... as columns of the projection
            const bool fold = p.ln_stats != nullptr;   // folded LayerNorm of the operand
            float cv[8] = {}, bv[8], x[8], v[8];
            if (fold) load8<float>(p.ln_c + n, cv);
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = site_x(e < 4 ? acc[0][2 * JP][e] : acc[0][2 * JP + 1][e - 4], os, fold, ln_rs[0], ln_mu[0], cv[e]);
            load8<float>(p.bias + n, bv);
            if (seg < 2) {                             // q / k: the row-major epilogue's values, K's row layout (Q behind K and V^T)
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = site_row_value(x[e], bv[e]);
                attn_store_row8<L>(smem + (seg ? 0 : L::BYTES), fm, cc, v, p.h2s);
            } else {                                   // v: the V^T epilogue's values, the V^T layout
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = site_vt_value(x[e], bv[e]);
                attn_store_vt8<L>(smem, fm, cc, v, p.h2s);
            }
        });
    };
    gemm_h2_tile<QA_BM, QA_BN, QA_WM, QA_WN, QA_NS, false, false, 1, true, false, 3>(p, b * QA_T, h * QA_HD, smem, 0, epi);
    __syncthreads();
    const int wave = (int)(threadIdx.x >> 6);
    if (wave >= QA_T / 16) return;
    AttnArgs a{nullptr, nullptr, nullptr, q.out, 0, 0, 0, 0, q.ldo, p.M / QA_T, QA_H, QA_T, QA_T, 1.0f / sqrtf((float)QA_HD), nullptr, p.h2s, p.h2i};
    attn_tile<float, QA_HD, 4, 1, true, true, true, true>(a, b, h, wave, 0, smem);
}

// what the site adds to the shared refusals (attn_site.h): its shape; the projection is the packed in_proj, N = 3 d
int make_problem(int dtype, const emage_qkv_attention_problem& q, int T, int d, int H, const H2Scale& hs, QkvAttnArgs& r) {
    if (T != QA_T || d != QA_D || H != QA_H) return EMAGE_EINVAL;
    const int rc = site_check(dtype, q, T, d);
    if (rc) return rc;
    r.g = site_projection(q, T, 3 * d, d, hs);
    r.out = q.out; r.ldo = q.ldo;
    return 0;
}

}  // namespace

extern "C" int emage_qkv_attention_grouped(int dtype, const emage_qkv_attention_problem* problems, int n_problems, int T, int d, int H, void* stream) {
    const auto make = [=](int dt, const emage_qkv_attention_problem& q, const H2Scale& hs, QkvAttnArgs& r) { return make_problem(dt, q, T, d, H, hs, r); };
    return launch_sites(dtype, problems, n_problems, H, make, qkv_attn_kernel, QA_THREADS, (hipStream_t)stream);
}

extern "C" int emage_qkv_attention(int dtype, const void* A, int lda, const void* W, const float* bias, const float* ln_stats, const float* ln_c,
                                   float ln_eps, void* out, int ldo, int B, int T, int d, int H, float a_scale, float w_scale, void* stream) {
    const emage_qkv_attention_problem q{A, W, bias, ln_stats, ln_c, out, lda, ldo, B, a_scale, w_scale, ln_eps};
    return emage_qkv_attention_grouped(dtype, &q, 1, T, d, H, stream);
}
