// emage_q_attention — one cross-attention site of the EMAGE decoder layers (T = Tk = 64 frames, d = 768, 4 heads of 192) as ONE launch
// instead of the q projection (emage_gemm, config 120 / 1120: a (B T, d) float32 q to memory) followed by emage_attention (which reads it
// straight back; nothing else ever does).  One workgroup per (clip, head), the skeleton of qkv_attention.hip:
//   * K-loop: gemm_h2_tile (h2_tile.h) unchanged on the 64 x 192 block tile of head h (its 192 W rows are contiguous in the packed q
//     projection) — wave rows of 32 (WM = 2) as in config 1120, so the folded LayerNorm's statistics merge in the same order; eight waves
//     of 32 x 48 on a ring of 3 (measured: 28.3-28.7 us per launch at 64 clips; four waves of 32 x 96: 31.3, rings of 2 / 4: 29.4 / 29.0; the
//     K / V^T loads issued in front of the K-loop and split behind it: 28.6, not faster — profiles/r10_q_attention_kernel_variants.txt);
//   * epilogue: the arithmetic of h2_tile_epilogue's float32 path for these columns (o_scale, the LayerNorm fold, bias), split into fp16
//     planes in LDS in the layout attn_stage_kv gives K (one row per query);
//   * K / V^T: float32 views of the layer's projected memory, staged by attn_stage_kv once the K-loop has released the operand ring
//     (K, V^T and Q together are 149 KiB: they fit the CU only without the ring);
//   * attention: attn_tile on LDS fragments (QLDS), four waves of 16 queries; `att` is written as the EMAGE_H2 image.
// Every q value, every split plane and the order of every MFMA over its contraction are those of the two-launch sequence: the output is
// the same bits (tests/test_q_attention_gpu.py).
// emage_qm_attention (second kernel below): the same site computing the layer's memory K / V^T itself, for the two decoder stacks.
#include "common.h"
#include <math.h>
#include "h2_tile.h"
#include "attn_tile.h"
#include "attn_site.h"

namespace emage_dev {

constexpr int CA_T = 64, CA_HD = 192, CA_H = 4, CA_D = CA_H * CA_HD;
constexpr int CA_BM = 64, CA_BN = CA_HD, CA_WM = 2, CA_WN = 4, CA_NS = 3;
constexpr int CA_THREADS = CA_WM * CA_WN * 64;
constexpr int CA_MAXG = 4;

struct QAttnArgs {
    GemmArgs g;                              // the projection as emage_gemm runs it (M = B T, N = K = d; no outputs of its own)
    const float* k; const float* vt;         // this layer's memory keys (B Tk, ldk) and V^T (B, vt_rows, ldvt), float32
    void* out;                               // att: (B T, ldo) EMAGE_H2 image
    int ldk, ldvt, vt_rows, ldo;
};
using QAttnGroup = SiteGroup<QAttnArgs, CA_MAXG>;

// emage_qm_attention: the site computes its memory K / V^T itself (see the kernel below)
constexpr int QM_BN = 2 * CA_HD, QM_NS = 2;
struct QmAttnArgs {
    GemmArgs g;                              // the q projection, as in QAttnArgs
    GemmArgs kv;                             // the stacked k|v projection of the memory features as emage_gemm runs it (M = B Tk, N = 2 layers d, K = km)
    int layer;                               // this site's layer in the stack: W rows [layer d, (layer + 1) d) are its keys, those N / 2 further on its values
    void* out; int ldo;                      // att: (B T, ldo) EMAGE_H2 image
};
using QmAttnGroup = SiteGroup<QmAttnArgs, CA_MAXG>;

}  // namespace emage_dev

namespace {

using namespace emage_dev;
using L = AttnLds<CA_HD, 4>;
constexpr int CA_LDS = L::BYTES + L::K_BYTES;            // K | V^T | Q planes

static_assert(h2_smem_bytes<CA_BM, CA_BN, CA_NS>() <= CA_LDS && CA_LDS <= 160 * 1024, "the operand ring lies inside the staged planes: one block per CU");

// The q projection's epilogue: q of this wave's 32 frames x WTN columns of head h -> split planes in LDS, K's row layout at smem + L::BYTES.
// Synchronises the workgroup before its first LDS store (the operand ring lies under the planes).
template <class Acc, class Stat>
__device__ __forceinline__ void q_planes(const GemmArgs& p, const int h, unsigned char* smem, Acc& acc, const int wm, const int wn, const int fr, const int fg,
                                         const Stat& ln_mu, const Stat& ln_rs) {
    constexpr int WTN = CA_BN / CA_WN, FN = WTN / 16;
    constexpr int NP = FN / 2;                     // fragment pairs (8 consecutive columns per lane); an odd FN leaves a lone fragment (4 columns)
    constexpr bool LONE = (FN & 1) != 0;
    // every bias / c value of the lane is requested before the barrier: one memory latency, not one per fragment
    const bool fold = p.ln_stats != nullptr;
    const int n0 = h * CA_HD + wn * WTN + fg * 8, nl = h * CA_HD + wn * WTN + (FN - 1) * 16 + fg * 4;
    float cv[NP][8], bv[NP][8];
    float4 cl = make_float4(0.f, 0.f, 0.f, 0.f), bl = cl;
    static_for<NP>([&](auto jc) {
        constexpr int JP = decltype(jc)::value;
        if (fold) load8<float>(p.ln_c + n0 + JP * 32, cv[JP]);
        load8<float>(p.bias + n0 + JP * 32, bv[JP]);
    });
    if constexpr (LONE) {
        if (fold) cl = *(const float4*)(p.ln_c + nl);
        bl = *(const float4*)(p.bias + nl);
    }
    __syncthreads();                               // every wave has read its last fragments of the ring
    const float os = p.o_scale;
    auto value = [&](const float accv, const float c, const float bias, const float mu, const float rs) { return site_row_value(site_x(accv, os, fold, rs, mu, c), bias); };
    static_for<2 * NP>([&](auto ic) {
        constexpr int I = decltype(ic)::value / NP, JP = decltype(ic)::value % NP;
        const int fm = wm * 32 + I * 16 + fr;      // frame of this lane's row
        const int cc = wn * WTN + JP * 32 + fg * 8;             // this lane's 8 columns inside the head: cc .. cc + 7
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = value(e < 4 ? acc[I][2 * JP][e] : acc[I][2 * JP + 1][e - 4], cv[JP][e], bv[JP][e], ln_mu[I], ln_rs[I]);
        attn_store_row8<L>(smem + L::BYTES, fm, cc, v, p.h2s);
    });
    if constexpr (LONE) {
        // the lone fragment (natural W row order): 4 consecutive columns per lane, one half of one cell
        static_for<2>([&](auto ic) {
            constexpr int I = decltype(ic)::value;
            const int fm = wm * 32 + I * 16 + fr;
            const int cc = wn * WTN + (FN - 1) * 16 + fg * 4;
            const float c4[4] = {cl.x, cl.y, cl.z, cl.w}, b4[4] = {bl.x, bl.y, bl.z, bl.w};
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = value(acc[I][FN - 1][e], c4[e], b4[e], ln_mu[I], ln_rs[I]);
            attn_store_row4<L>(smem + L::BYTES, fm, cc, v, p.h2s);
        });
    }
}

__global__ __launch_bounds__(CA_THREADS, 1) void q_attn_kernel(QAttnGroup g) {
    __shared__ __attribute__((aligned(128))) unsigned char smem[CA_LDS];
    int b, h;
    const QAttnArgs& q = site_block<CA_H>(g, b, h);
    const GemmArgs& p = q.g;
    const AttnArgs a{nullptr, q.k, q.vt, q.out, 0, q.ldk, q.ldvt, q.vt_rows, q.ldo, p.M / CA_T, CA_H, CA_T, CA_T, 1.0f / sqrtf((float)CA_HD), nullptr, p.h2s, p.h2i};

    auto epi = [&](auto& acc, const int, const int wm, const int wn, const int fr, const int fg, const auto& ln_mu, const auto& ln_rs) {
        q_planes(p, h, smem, acc, wm, wn, fr, fg, ln_mu, ln_rs);
    };
    gemm_h2_tile<CA_BM, CA_BN, CA_WM, CA_WN, CA_NS, false, false, 1, true, false, 1>(p, b * CA_T, h * CA_HD, smem, 0, epi);
    attn_stage_kv<CA_HD, 4, true, CA_THREADS>(a, b, h, smem);      // the ring is free: every wave passed the epilogue's barrier
    __syncthreads();
    const int wave = (int)(threadIdx.x >> 6);
    if (wave >= CA_T / 16) return;
    attn_tile<float, CA_HD, 4, 1, true, true, true, true>(a, b, h, wave, 0, smem);
}

// emage_qm_attention — the same site when the layer's memory K / V^T are themselves a projection of a narrow feature image (the audio features of the
// two decoder stacks, whose memory projection is composed with the K / V projections at packing time): the workgroup computes K_h / V_h of its clip
// itself instead of reading float32 K / V^T that one large emage_gemm wrote for every layer.
//   * k|v K-loop: gemm_h2_tile on a 64 x 384 block tile (SEGS = 2: the 192 key rows and the 192 value rows of head h of layer `layer` in the stacked
//     [K_0 .. K_n | V_0 .. V_n] operand), eight waves of 32 x 96 on a ring of 2 (112 KiB), K = km (256 / 512); the accumulators stay in registers;
//   * q K-loop and the q planes: q_attn_kernel's;
//   * k / v planes: the arithmetic of emage_gemm's float32 row-major (k) and V^T (v) epilogues (attn_site.h), split as attn_stage_kv splits the
//     float32 values it reads, into the layout it gives them (attn_tile.h: attn_store_row8 / attn_store_vt8; qkv_attention.hip does the same);
//   * attention: as above.
// `att` is the same bits as emage_gemm (K float32, V^T float32) + emage_q_attention (tests/test_qm_attention_gpu.py).
static_assert(h2_smem_bytes<CA_BM, QM_BN, QM_NS>() <= CA_LDS, "the k|v operand ring lies inside the staged planes");
static_assert(sizeof(QmAttnGroup) <= 4096, "the argument block travels in the kernarg segment");

__global__ __launch_bounds__(CA_THREADS, 1) void qm_attn_kernel(QmAttnGroup g) {
    constexpr int KWTN = QM_BN / CA_WN, KFN = KWTN / 16, KNP = KFN / 2;
    static_assert(KFN % 2 == 0 && CA_HD % KWTN == 0, "a wave's k|v columns are whole fragment pairs of k or of v");
    __shared__ __attribute__((aligned(128))) unsigned char smem[CA_LDS];
    int b, h;
    const QmAttnArgs& q = site_block<CA_H>(g, b, h);
    const GemmArgs& p = q.g;
    const GemmArgs& kv = q.kv;
    const int nkv0 = q.layer * CA_D + h * CA_HD;       // first key row of this head in the stacked operand; its values lie kv.N / 2 rows further on

    // k|v of this wave's 32 memory frames x 96 columns: kept until the q projection has run
    f32x4 kva[CA_BM / CA_WM / 16][KFN];
    auto keep = [&](auto& acc, const int, const int, const int, const int, const int, const auto&, const auto&) {
        static_for<CA_BM / CA_WM / 16>([&](auto ic) { static_for<KFN>([&](auto jc) { kva[decltype(ic)::value][decltype(jc)::value] = acc[decltype(ic)::value][decltype(jc)::value]; }); });
        __syncthreads();                               // every wave has read its last fragments: the q projection's DMA may overwrite the ring
    };
    gemm_h2_tile<CA_BM, QM_BN, CA_WM, CA_WN, QM_NS, false, false, 1, false, false, 2>(kv, b * CA_T, nkv0, smem, 0, keep);

    auto epi = [&](auto& acc, const int, const int wm, const int wn, const int fr, const int fg, const auto& ln_mu, const auto& ln_rs) {
        const int seg = wn * KWTN >= CA_HD ? 1 : 0;    // this wave holds keys / values (wave-uniform)
        const int c0 = wn * KWTN - seg * CA_HD + fg * 8;       // this lane's first column inside the head
        float kb[KNP][8];
        static_for<KNP>([&](auto jc) { load8<float>(kv.bias + seg * (kv.N / 2) + nkv0 + c0 + decltype(jc)::value * 32, kb[decltype(jc)::value]); });
        q_planes(p, h, smem, acc, wm, wn, fr, fg, ln_mu, ln_rs);         // (synchronises: the ring is free)
        const float os = kv.o_scale;
        static_for<2 * KNP>([&](auto ic) {
            constexpr int I = decltype(ic)::value / KNP, JP = decltype(ic)::value % KNP;
            const int fm = wm * 32 + I * 16 + fr;      // memory frame of this lane's row
            const int cc = c0 + JP * 32;               // this lane's 8 columns inside the head: cc .. cc + 7
            float v[8];
            if (seg == 0) {                            // k: the row-major epilogue's values, K's rows
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = site_row_value(site_x(e < 4 ? kva[I][2 * JP][e] : kva[I][2 * JP + 1][e - 4], os, false, 0.f, 0.f, 0.f), kb[JP][e]);
                attn_store_row8<L>(smem, fm, cc, v, p.h2s);
            } else {                                   // v: the V^T epilogue's values, the V^T rows
#pragma unroll
                for (int e = 0; e < 8; ++e) v[e] = site_vt_value(site_x(e < 4 ? kva[I][2 * JP][e] : kva[I][2 * JP + 1][e - 4], os, false, 0.f, 0.f, 0.f), kb[JP][e]);
                attn_store_vt8<L>(smem, fm, cc, v, p.h2s);
            }
        });
    };
    gemm_h2_tile<CA_BM, CA_BN, CA_WM, CA_WN, CA_NS, false, false, 1, true, false, 1>(p, b * CA_T, h * CA_HD, smem, 0, epi);
    __syncthreads();
    const int wave = (int)(threadIdx.x >> 6);
    if (wave >= CA_T / 16) return;
    const AttnArgs a{nullptr, nullptr, nullptr, q.out, 0, 0, 0, 0, q.ldo, p.M / CA_T, CA_H, CA_T, CA_T, 1.0f / sqrtf((float)CA_HD), nullptr, p.h2s, p.h2i};
    attn_tile<float, CA_HD, 4, 1, true, true, true, true>(a, b, h, wave, 0, smem);
}

// what the site adds to the shared refusals (attn_site.h): its shape and the layer's memory K / V^T with their limits; N = d
int make_problem(int dtype, const emage_q_attention_problem& q, int T, int Tk, int d, int H, const H2Scale& hs, QAttnArgs& r) {
    if (T != CA_T || Tk != CA_T || d != CA_D || H != CA_H) return EMAGE_EINVAL;
    const int rc = site_check(dtype, q, T, d);
    if (rc) return rc;
    if (!q.k || !q.vt || (((uintptr_t)q.k | (uintptr_t)q.vt) & 15)) return EMAGE_EINVAL;
    if (q.ldk % 4 || q.ldk < d || q.ldvt % 32 || q.ldvt < Tk || q.vt_rows < d) return EMAGE_EINVAL;
    if ((long)q.B * Tk * q.ldk * 4 >= (1L << 31) || (long)q.B * q.vt_rows * q.ldvt * 4 >= (1L << 31)) return EMAGE_EINVAL;
    r.g = site_projection(q, T, d, d, hs);
    r.k = q.k; r.vt = q.vt; r.out = q.out;
    r.ldk = q.ldk; r.ldvt = q.ldvt; r.vt_rows = q.vt_rows; r.ldo = q.ldo;
    return 0;
}

// emage_qm_attention: the memory feature image and the stacked k|v operand in place of K / V^T
int make_problem(int dtype, const emage_qm_attention_problem& q, int T, int Tk, int d, int H, const H2Scale& hs, QmAttnArgs& r) {
    if (T != CA_T || Tk != CA_T || d != CA_D || H != CA_H) return EMAGE_EINVAL;
    const int rc = site_check(dtype, q, T, d);
    if (rc) return rc;
    if (!q.mem || !q.Wkv || !q.bias_kv || (((uintptr_t)q.mem | (uintptr_t)q.Wkv | (uintptr_t)q.bias_kv) & 15)) return EMAGE_EINVAL;
    if (q.km < 32 || q.km % 32 || q.km > d || q.ldm % 8 || q.ldm < q.km || !(q.wkv_scale > 0.f)) return EMAGE_EINVAL;
    if (q.kv_layers < 1 || q.kv_layers > 64 || q.kv_layer < 0 || q.kv_layer >= q.kv_layers) return EMAGE_EINVAL;
    if ((long)q.B * Tk * q.ldm * 4 >= (1L << 31)) return EMAGE_EINVAL;
    r.g = site_projection(q, T, d, d, hs);
    r.kv = r.g;                                        // the same launch-wide fields; its own operands, contraction length and scale; no LayerNorm fold
    r.kv.A = q.mem; r.kv.W = q.Wkv; r.kv.bias = q.bias_kv;
    r.kv.lda = q.ldm;
    r.kv.N = 2 * q.kv_layers * d; r.kv.K = q.km; r.kv.Cp = q.km;
    r.kv.t_col0 = r.kv.N;
    r.kv.o_scale = 1.f / (q.a_scale * q.wkv_scale);
    r.kv.ln_stats = nullptr; r.kv.ln_np = 0; r.kv.ln_c = nullptr;
    r.layer = q.kv_layer;
    r.out = q.out; r.ldo = q.ldo;
    return 0;
}

}  // namespace

extern "C" int emage_q_attention_grouped(int dtype, const emage_q_attention_problem* problems, int n_problems, int T, int Tk, int d, int H, void* stream) {
    const auto make = [=](int dt, const emage_q_attention_problem& q, const H2Scale& hs, QAttnArgs& r) { return make_problem(dt, q, T, Tk, d, H, hs, r); };
    return launch_sites(dtype, problems, n_problems, H, make, q_attn_kernel, CA_THREADS, (hipStream_t)stream);
}

extern "C" int emage_q_attention(int dtype, const emage_q_attention_problem* problem, int T, int Tk, int d, int H, void* stream) {
    return emage_q_attention_grouped(dtype, problem, problem ? 1 : 0, T, Tk, d, H, stream);
}

extern "C" int emage_qm_attention_grouped(int dtype, const emage_qm_attention_problem* problems, int n_problems, int T, int Tk, int d, int H, void* stream) {
    const auto make = [=](int dt, const emage_qm_attention_problem& q, const H2Scale& hs, QmAttnArgs& r) { return make_problem(dt, q, T, Tk, d, H, hs, r); };
    return launch_sites(dtype, problems, n_problems, H, make, qm_attn_kernel, CA_THREADS, (hipStream_t)stream);
}

extern "C" int emage_qm_attention(int dtype, const emage_qm_attention_problem* problem, int T, int Tk, int d, int H, void* stream) {
    return emage_qm_attention_grouped(dtype, problem, problem ? 1 : 0, T, Tk, d, H, stream);
}
