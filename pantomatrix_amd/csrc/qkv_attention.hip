// emage_qkv_attention — one self-attention site of the EMAGE transformer layers (T = 64 frames, d = 768, 4 heads of 192) as ONE launch
// instead of the qkv projection (emage_gemm, config 100 / 1100: q / k float32 and V^T float32 to memory) followed by emage_attention
// (which reads them back).  One workgroup per (clip, head): at T = 64 the projection's row tile IS one clip, and everything the attention
// of head h needs are the 3 x 192 output columns q_h, k_h, v_h of those 64 rows.
//   * K-loop: gemm_h2_tile (h2_tile.h) unchanged on a 64 x 576 block tile — the 576 W rows are the three 192-row slices of head h
//     (SEGS = 3) — 8 waves of 16 x 288 (WTM = 16 as in config 100, so the folded LayerNorm's statistics merge in the same order);
//   * epilogue: the arithmetic of h2_tile_epilogue for these columns (o_scale, the LayerNorm fold, bias; q / k as the row-major float32
//     path computes them, v as the V^T path does), then split into fp16 planes straight into the operand ring, in the layout
//     attn_stage_kv gives K / V^T (and K's layout for Q);
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
    // XCD-aware order over the whole grid (gemm_h2_group_kernel): each XCD walks a contiguous run of (clip, head) blocks, heads fastest
    const int bid = xcd_run_order((int)blockIdx.x, g.total);
    int pi = 0;
#pragma unroll
    for (int i = 0; i < QA_MAXG - 1; ++i) pi += (i + 1 < g.n && bid >= g.blk_end[i]) ? 1 : 0;
    pi = __builtin_amdgcn_readfirstlane(pi);
    const int t = bid - (pi ? g.blk_end[pi - 1] : 0);
    const QkvAttnArgs& q = g.p[pi];
    const GemmArgs& p = q.g;
    const int b = t / QA_H, h = t - b * QA_H;

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
            float x[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = (e < 4 ? acc[0][2 * JP][e] : acc[0][2 * JP + 1][e - 4]) * os;
            if (p.ln_stats) {                          // folded LayerNorm of the operand
                float cv[8];
                load8<float>(p.ln_c + n, cv);
#pragma unroll
                for (int e = 0; e < 8; ++e) x[e] = ln_rs[0] * (x[e] - ln_mu[0] * cv[e]);
            }
            float bv[8];
            load8<float>(p.bias + n, bv);
            float v[8];
            uint4 hi, lo;
            if (seg < 2) {
                // q / k: the row-major epilogue's float32 values (no slope, no residual: leaky(., 1), + 0), split as attn_tile splits them
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float y = x[e] + bv[e];
                    y = leaky(y, 1.f);
                    y += 0.f;
                    v[e] = y;
                }
                h2_split8(v, hi, lo, p.h2s);
                // K / Q layout: row fm, cell (cc / 32, ((cc % 16) / 4)) holds columns 32 s + 4 g + r (planes [0, 4)) and 32 s + 16 + 4 g + r ([4, 8));
                // columns cc .. cc + 3 and cc + 4 .. cc + 7 fill the same half of two neighbouring cells
                unsigned char* dst = smem + (seg ? 0 : L::BYTES) + fm * L::KROW + (cc >> 5) * 128 + ((cc & 15) >> 2) * 32 + ((cc & 31) >> 4) * 8;
                *(uint2*)dst = make_uint2(hi.x, hi.y);
                *(uint2*)(dst + 16) = make_uint2(lo.x, lo.y);
                *(uint2*)(dst + 32) = make_uint2(hi.z, hi.w);
                *(uint2*)(dst + 48) = make_uint2(lo.z, lo.w);
            } else {
                // v: the V^T epilogue's values (leaky(acc + b, 1)), split into the V^T layout of attn_stage_kv (H2OUT row order): d row
                // 32 (dt >> 1) + 4 (dt & 1) + 8 (f >> 2) + (f & 3) is staged row 16 dt + f; key fm sits in cell (fm / 32, (fm % 16) / 4), slot
                // 4 ((fm % 32) / 16) + fm % 4
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = leaky(x[e] + bv[e], 1.f);
                h2_split8(v, hi, lo, p.h2s);
                const h2f16x8 hv = __builtin_bit_cast(h2f16x8, hi), lv = __builtin_bit_cast(h2f16x8, lo);
                unsigned char* col = smem + L::K_BYTES + ((fm >> 5) * 4 + ((fm & 15) >> 2)) * 32 + (((fm & 31) >> 4) * 4 + (fm & 3)) * 2;
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const int j = 16 * (2 * (cc >> 5) + (e >> 2)) + 4 * ((cc & 31) >> 3) + (e & 3);
                    *(_Float16*)(col + j * L::VROW) = hv[e];
                    *(_Float16*)(col + j * L::VROW + 16) = lv[e];
                }
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

int qkv_attention_impl(int dtype, const emage_qkv_attention_problem* problems, int n, int T, int d, int H, hipStream_t s) {
    const auto make = [=](int dt, const emage_qkv_attention_problem& q, const H2Scale& hs, QkvAttnArgs& r) { return make_problem(dt, q, T, d, H, hs, r); };
    return launch_sites(dtype, problems, n, H, make, qkv_attn_kernel, QA_THREADS, s);
}

}  // namespace

extern "C" int emage_qkv_attention(int dtype, const void* A, int lda, const void* W, const float* bias, const float* ln_stats, const float* ln_c,
                                   float ln_eps, void* out, int ldo, int B, int T, int d, int H, float a_scale, float w_scale, void* stream) {
    emage_qkv_attention_problem q{A, W, bias, ln_stats, ln_c, out, lda, ldo, B, a_scale, w_scale, ln_eps};
    return qkv_attention_impl(dtype, &q, 1, T, d, H, (hipStream_t)stream);
}

extern "C" int emage_qkv_attention_grouped(int dtype, const emage_qkv_attention_problem* problems, int n_problems, int T, int d, int H, void* stream) {
    return qkv_attention_impl(dtype, problems, n_problems, T, d, H, (hipStream_t)stream);
}
