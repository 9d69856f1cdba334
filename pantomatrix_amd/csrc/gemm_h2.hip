// emage_gemm, EMAGE_H2 mode: Linear / Conv1d as implicit GEMM over PRE-SPLIT operands (h2.h) — the parity-green split-fp16
// MFMA arithmetic of EMAGE_F16X3 (hi*hi + hi*lo + lo*hi, fp32 accumulate) with the activation split done ONCE by the producer
// instead of by every consuming wave at every K-tile.  Tile routine: h2_tile.h.
#include "common.h"
#include <utility>
#include "h2_tile.h"

namespace emage_dev {
#ifdef EMAGE_TOOLS
int g_h2_force_config = -1;      // tools build (emage_set_tuning key 4): fixed tile configuration for sweeps
int g_h2_variant = 0;            // tools build: dispatch-heuristic variant for A/B runs (emage_set_tuning key 5)
int g_h2_small_cfg = 0;          // tools build: tile configuration for grids of at most one 64 x 64 tile per CU (emage_set_tuning key 7; 0 = the shipped 120)
unsigned long long* g_h2_trace = nullptr;   // tools build: device buffer of (waves x 512) s_memtime stamps (emage_h2_set_trace)
#else
constexpr int g_h2_force_config = -1, g_h2_variant = 0, g_h2_small_cfg = 0;
constexpr unsigned long long* g_h2_trace = nullptr;
#endif
}

namespace {

using namespace emage_dev;

// One tile configuration: what gemm_h2_tile (h2_tile.h) takes as template arguments, by name
struct H2Tile {
    int bm, bn;                  // block tile
    int wm = 2, wn = 2;          // grid of waves (wave tile bm / wm x bn / wn)
    int ns = 3;                  // ring depth in K-tiles (2..4)
    int occ = 1;                 // resident blocks per CU the launch bounds ask for, in blocks of 4 waves
    bool dilv = false;           // DMA issue interleaved with the MFMAs
    bool trace = false;          // phase tracer
    int kpb = 1;                 // K-tiles per ring slot and barrier
    bool lnf = false;            // the LayerNorm-fold paths (GemmArgs::ln_stats / rs_stats / st_out)
    constexpr int waves() const { return wm * wn; }
    constexpr int threads() const { return waves() * 64; }
};
enum : int { GROUP = 1, FIXUP = 2 };
struct H2Row {
    int id;
    H2Tile t;
    int flags = 0;               // GROUP: has a grouped kernel (emage_gemm_grouped); FIXUP: has the split-K form with the in-kernel fix-up (SKF)
};

// THE tile configurations (id: block tile, wave grid [wave tile], ring depth, K-loop form); every launcher, kernel and
// predicate below takes its row from here.  The product library carries the rows the heuristics select; the rest are the tools build's
constexpr H2Row H2_CONFIGS[] = {
    {100, {.bm = 64, .bn = 192, .wm = 4, .ns = 2}, GROUP},                    // 8 waves 16x96 (the F16X3 shape)
    {170, {.bm = 128, .bn = 192, .wn = 4, .ns = 2}, GROUP},                   // 8 waves 64x48: grids of many tiles per CU (round 4)
    {113, {.bm = 128, .bn = 128, .wm = 4}, GROUP},
    {119, {.bm = 128, .bn = 256, .wm = 4, .ns = 2}, GROUP},                   // 8 waves 32x128
    {120, {.bm = 64, .bn = 64, .occ = 2}, GROUP | FIXUP},                     // 768-wide / small outputs: 4 waves 32x32, three blocks per CU
    // the same two tiles WITH the LayerNorm-fold paths (GemmArgs::ln_stats / rs_stats / st_out; round 6): taken only by launches that fold
    {1100, {.bm = 64, .bn = 192, .wm = 4, .ns = 2, .lnf = true}, GROUP},
    {1120, {.bm = 64, .bn = 64, .occ = 2, .lnf = true}, GROUP | FIXUP},
#ifdef EMAGE_TOOLS
    {101, {.bm = 64, .bn = 192, .wm = 4}},
    {102, {.bm = 64, .bn = 192, .wn = 4}},                                    // 8 waves 32x48
    {112, {.bm = 128, .bn = 128, .wm = 4, .ns = 2}},                          // 8 waves 32x64
    {116, {.bm = 128, .bn = 192, .wm = 4}},                                   // 8 waves 32x96
    {189, {.bm = 64, .bn = 64, .wn = 4}},                                     // round 5: the same tile on 8 waves of 32 x 16 (2 DMA instructions per wave and K-tile instead of 4)
    {130, {.bm = 64, .bn = 64, .ns = 2, .occ = 3}},
    // DMA issue interleaved with the MFMAs (DILV)
    {140, {.bm = 64, .bn = 192, .wm = 4, .ns = 2, .dilv = true}},
    {141, {.bm = 64, .bn = 192, .wm = 4, .dilv = true}},
    {142, {.bm = 64, .bn = 192, .wn = 4, .dilv = true}},
    {145, {.bm = 128, .bn = 128, .wm = 4, .dilv = true}},
    {147, {.bm = 128, .bn = 192, .wm = 4, .dilv = true}},
    {149, {.bm = 128, .bn = 256, .wm = 4, .ns = 2, .dilv = true}},
    {150, {.bm = 64, .bn = 64, .ns = 2, .occ = 3, .dilv = true}},
    {151, {.bm = 64, .bn = 64, .occ = 2, .dilv = true}},
    {152, {.bm = 128, .bn = 64, .wm = 4, .dilv = true}},                      // 8 waves 32x32
    {153, {.bm = 64, .bn = 128, .wn = 4, .dilv = true}},                      // 8 waves 32x32
    {155, {.bm = 64, .bn = 192, .wm = 4, .ns = 4, .dilv = true}},
    {156, {.bm = 128, .bn = 128, .wn = 4, .dilv = true}},                     // 8 waves 64x32
    // round 4: FEWER waves with larger wave tiles (LDS fragment bytes per MFMA fall with the wave tile: a 32x32 wave tile reads 8 KB per
    // 12 MFMAs, a 64x48 one 14 KB per 36), several blocks per CU
    {160, {.bm = 64, .bn = 96, .wm = 1, .occ = 2}, GROUP},                    // 2 waves 64x48, two blocks per CU
    {162, {.bm = 64, .bn = 64, .wm = 1, .occ = 3}, GROUP},                    // 2 waves 64x32, three blocks per CU
    {163, {.bm = 64, .bn = 64, .wn = 1, .occ = 3}, GROUP},                    // 2 waves 32x64
    {165, {.bm = 64, .bn = 64, .wm = 1, .wn = 1, .occ = 3}},
    {166, {.bm = 128, .bn = 96}},                                             // 4 waves 64x48, one block per CU
    {168, {.bm = 64, .bn = 192, .wm = 1, .wn = 4}},                           // 4 waves 64x48 side by side
    {171, {.bm = 128, .bn = 256, .wn = 4, .ns = 2}},                          // 8 waves 64x64
    // round 5: one fat block per CU for grids of many tiles per CU (the K / V projections of all cross-attention layers): MFMA issue per K-tile
    // 3-4x the operand delivery (64 B/clk per CU)
    {172, {.bm = 256, .bn = 256, .wn = 4, .ns = 2}},                          // 8 waves 128x64
    {173, {.bm = 256, .bn = 192, .wn = 4, .ns = 2}},                          // 8 waves 128x48
    {174, {.bm = 256, .bn = 192, .wm = 4, .ns = 2}},                          // 8 waves 64x96
    {175, {.bm = 256, .bn = 128, .wm = 4, .ns = 2}},                          // 8 waves 64x64
    // round 5 (VERDICT next #1b, "BK = 64"): TWO K-tiles per ring slot and barrier (KPB = 2), otherwise the shipped configurations
    {180, {.bm = 64, .bn = 192, .wm = 4, .ns = 2, .kpb = 2}},                 // 100 with 128 KB of LDS: one block per CU
    {181, {.bm = 128, .bn = 192, .wn = 4, .ns = 2, .kpb = 2}},                // 170 with 160 KB: one block per CU instead of two
    {183, {.bm = 64, .bn = 64, .ns = 2, .occ = 2, .kpb = 2}},                 // 120 with a ring of 2 x 32 KB: two blocks per CU
    {184, {.bm = 128, .bn = 128, .wm = 4, .ns = 2, .kpb = 2}},                // 113 with a ring of 2 x 64 KB
    {185, {.bm = 64, .bn = 128, .wn = 4, .ns = 2, .kpb = 2}},                 // 8 waves 32x32, 96 KB
    {186, {.bm = 64, .bn = 64, .kpb = 2}},                                    // 120's ring of 3, 96 KB: one block per CU
    // instrumented twins (TRACE) of 101 / 141
    {201, {.bm = 64, .bn = 192, .wm = 4, .trace = true}},
    {241, {.bm = 64, .bn = 192, .wm = 4, .dilv = true, .trace = true}},
#endif
};
static_assert(unique_config_ids<H2_CONFIGS>(), "one row per id");
constexpr bool h2_rows_consistent() {
    for (const H2Row& r : H2_CONFIGS) {
        if ((r.flags & (GROUP | FIXUP)) && (r.t.kpb != 1 || r.t.trace)) return false;      // launch_h2_group / launch_h2_skf check no K-tile parity and pass no trace buffer
        if ((r.flags & FIXUP) && (r.t.bm != 64 || r.t.bn != 64)) return false;            // h2_skf_slices plans 64 x 64 tiles
    }
    return true;
}
static_assert(h2_rows_consistent(), "a GROUP / FIXUP row the grouped or fix-up launch cannot run");
static const H2Row* h2_row(int id) {
    for (const H2Row& r : H2_CONFIGS) if (r.id == id) return &r;
    return nullptr;
}

template <H2Tile C, bool SKF>
__global__ __launch_bounds__(C.waves() * 64, C.occ * C.waves() / 4) void gemm_h2_kernel(GemmArgs p) {
    __shared__ __attribute__((aligned(128))) unsigned char smem[h2_smem_bytes<C.bm, C.bn, C.ns, C.kpb>()];
    // XCD-aware tile order (gemm_tile.h): each XCD walks a contiguous run of tiles; split-K: slice s = blockIdx / tiles
    const int nblk = p.tiles_m * p.tiles_n;
    const int split = p.ksplit > 1 ? (int)blockIdx.x / nblk : 0;
    int bid = (int)blockIdx.x - split * nblk;
    if (p.tile_order == 0 && !EMAGE_DBG(p, 32)) bid = xcd_run_order(bid, nblk);     // (tools: emage_set_tuning key 1 bit 32, tools/prof_traffic_calib.py: dispatch order for every launch)
    int tile_n = bid % p.tiles_n, tile_m = bid / p.tiles_n;
    if (EMAGE_DBG(p, 64)) { tile_m = bid % p.tiles_m; tile_n = bid / p.tiles_m; }      // tools: an XCD's run walks M first (it owns a slice of N: A re-fetched per XCD, W once)
    gemm_h2_tile<C.bm, C.bn, C.wm, C.wn, C.ns, C.dilv, C.trace, C.kpb, C.lnf, SKF>(p, tile_m * C.bm, tile_n * C.bn, smem, split);
}


// most tiles a split-K launch may have: 100.  Measured on the captured training step (A/Bs on one box each, tools library variants):
//   * 384 instead of 191 (the 768 x 1536 FFN weight gradients: 288 tiles -> two slices of 576 blocks): 105.2 -> 109.6 ms
//     (profiles/r04_train_step_ab_splitk_accumulate.txt) — the second slice's atomic epilogue costs more than the idle block slots;
//   * no split-K at all: 103.4 -> 119.0 ms (the 48- / 96-tile gradients of the heads and narrow MLPs need it);
//   * 100 instead of 191: 103.4 -> 98.4 ms (profiles/r04_train_step_ab_splitk_limit.txt) — the 144-tile 768 x 768 weight gradients (three
//     per decoder layer) run 80 us as four atomically-added slices and ~45 us as one slice per block on 144 CUs
//     (profiles/r04_gemm_h2_sweep_backward_shapes.txt: the 288-tile gradient, twice the work and never split, takes 47.5 us).
// Tools build: emage_set_tuning key 5 bit 1024 selects 384, bit 2048 no split-K, bit 4096 round 3's 191 (A/B runs)
static inline long h2_split_k_tiles() { return (g_h2_variant & 1024) ? 384 : (g_h2_variant & 2048) ? -1 : (g_h2_variant & 4096) ? 191 : 100; }
static inline bool h2_accumulates_in_place(const GemmArgs& a) {
    return a.res && a.res_is_f32 && a.out_f32 && (const void*)a.res == (const void*)a.out_f32 && a.ldr == a.ldf;
}
// A "bare" contraction, the only kind split-K (atomic or two-pass) may cut into K-slices: only out_f32 (optionally accumulating in place),
// no bias / activation / residual, no LayerNorm fold and no row statistics out — a slice's epilogue sees its partial sums only (the
// weight gradients of a training step), and K >= 2048.
static inline bool h2_bare(const GemmArgs& a) {
    return a.taps == 1 && !a.out && !a.out_t && (!a.res || h2_accumulates_in_place(a)) && !a.bias && !a.slope && a.out_f32 &&
           !a.ln_stats && !a.rs_stats && !a.st_out && a.K / 32 >= 64;
}

// second pass of a workspace split-K: out[m][n] (+)= plane_0[m][n] + plane_1[m][n] + ... in slice order — a fixed association, so the
// result is the same bits on every run (the atomic form adds the slices in arrival order).  4 columns per thread.
__global__ __launch_bounds__(256) void h2_splitk_reduce_kernel(const float* __restrict__ ws, long plane, int ldws, int nslices,
                                                               float* __restrict__ out, int ldf, int M, int N, int accumulate) {
    const int n4 = (N + 3) >> 2;
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= (long)M * n4) return;
    const int m = (int)(t / n4), n = (int)(t - (long)m * n4) << 2;
    const bool vec = n + 4 <= N && (ldf & 3) == 0 && (((uintptr_t)out & 15) == 0);
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    float* dst = out + (long)m * ldf + n;
    if (accumulate) {
        if (vec) { const float4 q = *(const float4*)dst; v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; }
        else { for (int e = 0; e < 4; ++e) if (n + e < N) v[e] = dst[e]; }
    }
    const float* src = ws + (long)m * ldws + n;          // ldws % 4 == 0 and the planes are 16-byte aligned: whole float4s (columns >= N hold zeros or junk, never stored)
    for (int s = 0; s < nslices; ++s) {
        const float4 q = *(const float4*)(src + (long)s * plane);
        v[0] += q.x; v[1] += q.y; v[2] += q.z; v[3] += q.w;
    }
    if (vec) *(float4*)dst = make_float4(v[0], v[1], v[2], v[3]);
    else { for (int e = 0; e < 4; ++e) if (n + e < N) dst[e] = v[e]; }
}

// CU count the heuristics plan for: the current device's (256 on MI355X; the fallback when the query fails)
static inline int h2_cus() { const int c = device_cus(); return c > 0 ? c : 256; }

// block slots of the chip for a tile configuration (LDS-bound residency x CUs of the current device): what a split-K launch should fill.
// The count only steers how many K-slices are cut, never correctness
template <H2Tile C>
int h2_block_slots() {
    constexpr int by_lds = (160 * 1024) / h2_smem_bytes<C.bm, C.bn, C.ns, C.kpb>();
    constexpr int by_waves = 32 / C.waves();
    return h2_cus() * (by_lds < by_waves ? (by_lds < 1 ? 1 : by_lds) : by_waves);
}

template <H2Tile C>
int launch_h2(GemmArgs& a, hipStream_t s) {
    if (!C.lnf && (a.ln_stats || a.rs_stats || a.st_out)) return EMAGE_EINVAL;      // only the LNF rows know the LayerNorm-fold fields
    if (a.out_t && a.t_col0 % C.bn != 0) return EMAGE_EINVAL;      // a tile is either row-major or transposed
    if (C.kpb > 1 && (a.K / 32) % C.kpb != 0) return EMAGE_EINVAL;   // a ring slot holds KPB whole K-tiles: an odd count would drop the last one
    set_tile_grid(a, C.bm, C.bn);
    a.trace = C.trace ? g_h2_trace : nullptr;
    // Tile order (round 5, profiles/r05_traffic_calibration.txt, r05_gemm_h2_tile_order_ab.txt).  XCD-aware runs keep an XCD's W panels in ITS L2 — as long
    // as W fits the eight 4 MB L2s next to the A panels.  The K / V projection of all cross-attention layers (W = 12 288 x 768 x 4 B = 37.7 MB) does not:
    // a strip-shaped run shares an A panel among its 64 concurrent blocks and a W panel among none (1 233 MB over the fabric, 3.9x the model); in
    // dispatch order consecutive tiles sit on different XCDs and every XCD works on the same few W panels at a time: 390 MB, 227 vs 242 us.  Smaller W
    // (qkv 7 MB: no difference; out_proj 2.4 MB: 4 % slower) keeps the runs.  Tools: emage_set_tuning key 5 bit 4194304 keeps the runs everywhere
    // Only the measured kind of launch takes it: a biased projection (no gradient contraction — those were never timed in dispatch order)
    a.tile_order = (!(g_h2_variant & 4194304) && a.bias && a.taps == 1 && (long)a.N * a.K * 4 >= (32L << 20)) ? 1 : 0;
    // split-K: a bare contraction (only out_f32, no bias / activation / residual — the weight gradients of a training step: few output
    // tiles, a very long K) with too few tiles to fill the chip is cut into K-slices whose partial tiles are atomically added in memory.
    a.ksplit = 1;
    const long tiles = (long)a.tiles_m * a.tiles_n;
    const int nk_all = a.K / 32;
    // res == out_f32 (fp32, same pitch): "out_f32 += contraction" — a weight gradient accumulated straight into the parameter's gradient.
    // One slice: the epilogue's residual add does it in place.  Split-K: the atomics land on the existing contents (no clearing, no residual)
    const bool accumulate = h2_accumulates_in_place(a);
    const bool bare = h2_bare(a);
    float* const ws = a.ws;
    const long ws_floats = a.ws_plane;                 // emage_gemm_ws: capacity of the workspace in floats (gemm.hip)
    a.ws = nullptr; a.ws_plane = 0; a.ldws = 0;
    bool reduce = false;
    if (bare && ws && !(g_h2_variant & 16384)) {      // tools A/B: bit 16384 = ignore the workspace (the atomic form)
        // two-pass split-K (emage_gemm_ws): as many K-slices as fill the chip's block slots ONCE, each slice >= 16 K-tiles, partial tiles as
        // planes of the workspace.  Cheap enough (plain stores + one streaming pass) to use up to twice the tile count of the atomic form
        const int SLOTS = h2_block_slots<C>();
        const int ldws = (a.N + 3) & ~3;
        const long plane = ((long)a.M * ldws + 3) & ~3L;
        int want = (int)(SLOTS / tiles);
        const int most = nk_all / 16;
        if (want > most) want = most;
        if (want > 16) want = 16;
        if (plane > 0 && (long)want * plane > ws_floats) want = (int)(ws_floats / plane);
        const long most_tiles = (g_h2_variant & 8192) ? 191 : SLOTS / 2;       // tools A/B: bit 8192 = two-pass below 192 tiles only
        if (want > 1 && tiles <= most_tiles) {
            int per = (nk_all + want - 1) / want;
            per = (per + 1) & ~1;
            a.nk_split = per;
            a.ksplit = (nk_all + per - 1) / per;
            if (a.ksplit > 1) {
                a.ws = ws; a.ws_plane = plane; a.ldws = ldws;
                a.res = nullptr;                       // an accumulating contraction: the reduce pass adds onto the destination
                reduce = true;
            } else {
                a.ksplit = 1;
            }
        }
    }
    if (!reduce && bare && tiles <= h2_split_k_tiles()) {     // no workspace (emage_gemm), or one too small for two slices: K-slices met by fp32 atomics
        int want = (int)((512 + tiles - 1) / tiles);
        const int most = nk_all / 16;                  // >= 16 K-tiles (512 k) per slice
        if (want > most) want = most;
        if (want > 64) want = 64;
        if (want > 1) {
            int per = (nk_all + want - 1) / want;
            per = (per + 1) & ~1;                      // K-tiles in pairs (the two-K-tiles-per-slot rows need an even count)
            a.nk_split = per;
            a.ksplit = (nk_all + per - 1) / per;
            if (accumulate) {
                a.res = nullptr;
            } else {
                const hipError_t e = hipMemset2DAsync(a.out_f32, (size_t)a.ldf * sizeof(float), 0, (size_t)a.N * sizeof(float), (size_t)a.M, s);
                if (e != hipSuccess) return (int)e;
            }
        }
    }
    hipLaunchKernelGGL((gemm_h2_kernel<C, false>), dim3(a.tiles_m * a.tiles_n * a.ksplit), dim3(C.threads()), 0, s, a);
    if (!reduce) return launch_status();
    const int rc = launch_status();
    if (rc) return rc;
    const long quads = (long)a.M * ((a.N + 3) >> 2);
    hipLaunchKernelGGL(h2_splitk_reduce_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, (const float*)a.ws, a.ws_plane, a.ldws, a.ksplit,
                       a.out_f32, a.ldf, a.M, a.N, accumulate ? 1 : 0);
    return launch_status();
}

// ---- split-K with the in-kernel fix-up (h2_tile.h SKF; round 6): few-row launches (ONE clip: M = 64 — 12 to 36 tiles of 64 x 64 that each
// walk their 24-48 K-tiles ALONE on a CU, profiles/r05_bench_kernel_stats_one_clip_serialized.csv) are cut into K-slices so that a launch
// occupies ~a block per CU; the last block of a tile to arrive sums the slices in slice order and runs the unchanged epilogue (every
// output form, the LayerNorm fold).  The 64 x 64 tile only.  Returns < 0: not applicable (the caller launches the plain form).
static int h2_skf_slices(const GemmArgs& a, int* per_out) {
    if (!a.sk_ws || !a.sk_count) return -1;
    const long tiles = tile_count(a, 64, 64);
    const int nk_all = a.K / 32;
    if (tiles > 128 || tiles > a.sk_tiles || nk_all < 8) return -1;
    int want = (int)((h2_cus() + tiles - 1) / tiles);          // ~one block per CU
    if (want > nk_all / 4) want = nk_all / 4;                  // >= 4 K-tiles per slice
    if (want > 16) want = 16;
    if (want < 2) return -1;
    const int per = (nk_all + want - 1) / want;
    const int ksplit = (nk_all + per - 1) / per;
    if (ksplit < 2 || tiles * ksplit * (64L * 64 * 4) > a.sk_ws_bytes) return -1;
    *per_out = per;
    return ksplit;
}
template <H2Tile C>
int launch_h2_skf(GemmArgs& a, int ksplit, int per, hipStream_t s) {
    if (a.out_t && a.t_col0 % C.bn != 0) return EMAGE_EINVAL;
    set_tile_grid(a, C.bm, C.bn);
    a.trace = nullptr;
    a.tile_order = 0;
    a.ws = nullptr; a.ws_plane = 0; a.ldws = 0;
    a.ksplit = ksplit; a.nk_split = per;
    hipLaunchKernelGGL((gemm_h2_kernel<C, true>), dim3(a.tiles_m * a.tiles_n * ksplit), dim3(C.threads()), 0, s, a);
    return launch_status();
}


// ---- grouped launch: several independent problems of ONE tile configuration in one grid (emage_gemm_grouped) ----
// The argument block carries the problems by value (kernarg segment: no device table to allocate); a block finds its problem by
// comparing its (XCD-remapped) id with the running tile counts — scalar work — and then runs the unchanged tile routine on that
// problem's arguments: the result is bit for bit that of the single-problem launch.


template <H2Tile C>
__global__ __launch_bounds__(C.waves() * 64, C.occ * C.waves() / 4) void gemm_h2_group_kernel(GroupArgs g) {
    __shared__ __attribute__((aligned(128))) unsigned char smem[h2_smem_bytes<C.bm, C.bn, C.ns, C.kpb>()];
    // XCD-aware order over the WHOLE grid: each XCD walks a contiguous run of the concatenated tile list, i.e. mostly one problem
    // (its W panel stays in that XCD's L2)
    const int bid = xcd_run_order((int)blockIdx.x, g.total);
    // which problem is this block in (written out here, in qkv_attention.hip and in q_attention.hip: moved into a shared function,
    // the same scan makes the compiler number these kernels' scalar registers differently)
    int pi = 0;
#pragma unroll
    for (int i = 0; i < MAXG - 1; ++i) pi += (i + 1 < g.n && bid >= g.tile_end[i]) ? 1 : 0;
    pi = __builtin_amdgcn_readfirstlane(pi);
    const int t = bid - (pi ? g.tile_end[pi - 1] : 0);
    const GemmArgs& p = g.p[pi];
    const int tile_n = t % p.tiles_n, tile_m = t / p.tiles_n;
    gemm_h2_tile<C.bm, C.bn, C.wm, C.wn, C.ns, C.dilv, C.trace, C.kpb, C.lnf>(p, tile_m * C.bm, tile_n * C.bn, smem, 0);
}

// the split-K condition of launch_h2 (bare contractions with few tiles and a long K: the weight gradients of a training step)
static bool h2_wants_split_k(const GemmArgs& a, const H2Tile& c) { return h2_bare(a) && tile_count(a, c.bm, c.bn) <= h2_split_k_tiles(); }

template <H2Tile C>
int launch_h2_group(GemmArgs** a, int n, hipStream_t s) {
    GroupArgs g;
    const int rc = fill_group(g, a, n, C.bm, C.bn);
    if (rc) return rc;
    hipLaunchKernelGGL((gemm_h2_group_kernel<C>), dim3(g.total), dim3(C.threads()), 0, s, g);
    return launch_status();
}

}  // namespace


#ifdef EMAGE_TOOLS
extern "C" int emage_h2_set_trace(void* buf) { emage_dev::g_h2_trace = (unsigned long long*)buf; return 0; }
#endif

namespace emage_dev {

// the tile configuration of one problem.  Measured on MI355X (tools/bench_gemm_h2.py, profiles/r03_h2_sweep*.txt).  Wide outputs: 8-wave
// 64x192 / 128x256 tiles; everything else: 64x64 tiles, three resident blocks per CU (their barriers de-synchronise, which hides each
// block's DMA / LDS phases behind the others' MFMAs better than one fat block per CU does at M = 4096).  < 0: unsupported argument
static int h2_config_for(const GemmArgs& a) {
    if (g_h2_force_config >= 0) return g_h2_force_config;
    const int ncols = store_cols(a);
    const int v = g_h2_variant;
    if ((v & 1) && ncols < 1024 && ncols % 192 == 0 && a.M >= 2048 && !a.out_t) return 101;       // one 8-wave block per CU
    if ((v & 16) && ncols < 1024 && ncols % 96 == 0 && a.M >= 2048 && !a.out_t) return 160;      // 64x96, two 2-wave blocks per CU
    if ((v & 64) && ncols < 1024 && !a.out_t) return 162;
    if ((v & 128) && ncols < 1024 && !a.out_t) return 163;
    if (ncols >= 1024 && a.M >= 1024) {
        const long t128x256 = tile_count(a, 128, 256);
        // many tiles per CU (the K/V projections of all cross-attention layers, N = 12288): 64x48 wave tiles read 14 KB of fragments per 36
        // MFMAs (the 32x128 ones of 119: 20 KB per 48) and two 80 KB blocks fit a CU: 239 vs 270 us (profiles/r04_gemm_h2_sweep_fewer_waves_wide.txt)
        const long t128x192 = tile_count(a, 128, 192);
        const long cus = h2_cus();                     // the thresholds were measured on 256 CUs: 4 / 2 tiles per CU
        if (!(v & 512) && t128x192 >= 4 * cus && ncols % 192 == 0 && (!a.out_t || a.t_col0 % 192 == 0)) return 170;
        if (!(v & 2) && t128x256 >= 2 * cus && ncols % 256 == 0 && (!a.out_t || a.t_col0 % 256 == 0)) return 119;
        if (ncols % 192 == 0 && (!a.out_t || a.t_col0 % 192 == 0)) return 100;
        if (!a.out_t || a.t_col0 % 128 == 0) return 113;
    }
    // 768-wide outputs of a LONG contraction over many rows (the K / V projections of all cross-attention layers in the backward of a training
    // step: dW 12288 x 768 and 6144 x 768 with K = 3584, dX 3584 x 768 with K = 12288 / 6144): many 64 x 64 tiles per block slot, each re-streaming
    // its operands — the 8-wave tiles move half the bytes per MFMA (profiles/r05_gemm_h2_sweep_backward_two_pass.txt: 187-197 vs 234-266 us,
    // 104-116 vs 133-134 us).  Below ~20 M (rows x k) the 64 x 64 tile wins (the window shapes of inference: M = 4096, K <= 1536)
    if (!(v & 65536) && !a.out_t && ncols % 192 == 0 && ncols >= 768 && a.taps == 1) {
        const long mk = (long)a.M * a.K, per_cu = 1000L * 1000 * h2_cus() / 256;     // measured on 256 CUs: 40 M / 20 M (rows x k)
        if (mk >= 40L * per_cu) return 170;
        if (mk >= 20L * per_cu) return 100;
    }
    if (a.out_t && a.t_col0 % 64 != 0) return EMAGE_EINVAL;
    return (v & 8) ? 130 : 120;
}

// a launch that folds a LayerNorm (operand statistics, a folded residual, statistics out) takes the LNF twin of its configuration — 100 / 120 only
static int h2_fold_config(const GemmArgs& a, int cfg) {
    if (!(a.ln_stats || a.rs_stats || a.st_out) || cfg < 0) return cfg;
    const int ncols = store_cols(a);
    if (a.st_out) return (a.out_t || ncols >= 1024) ? EMAGE_EINVAL : 1120;      // row statistics come out of the 64 x 64 tile's 32 x 32 wave tiles only
    if (cfg == 120 || cfg == 100) return cfg + 1000;
    // batches whose plain launch would take another tile (119 / 170 / 113 beyond ~7 000 rows): the fold exists in two tiles only
    if (ncols >= 1024 && ncols % 192 == 0 && (!a.out_t || a.t_col0 % 192 == 0)) return 1100;
    return (a.out_t && a.t_col0 % 64 != 0) ? EMAGE_EINVAL : 1120;
}

// one problem on configuration `cfg`, alone in its launch.  A FIXUP row with few rows and a fix-up workspace: split-K inside the launch
static int h2_launch_one(int cfg, GemmArgs& a, hipStream_t s) {
    return with_config<H2_CONFIGS>(cfg, [&]<H2Row R>() {
        if constexpr (R.flags & FIXUP) {
            int per = 0;
            const int ksplit = h2_skf_slices(a, &per);
            if (ksplit > 1) return launch_h2_skf<R.t>(a, ksplit, per, s);
        }
        return launch_h2<R.t>(a, s);
    });
}

// called by emage_gemm (gemm.hip) for dtype EMAGE_H2 after the common argument checks
int gemm_h2_dispatch(GemmArgs& a, hipStream_t s) {
    int cfg = h2_fold_config(a, h2_config_for(a));
#ifdef EMAGE_TOOLS
    if (cfg == 120 && g_h2_force_config < 0 && ((g_h2_variant & 1048576) || g_h2_small_cfg > 0)) {       // tools A/B: lone-block grids on 8 waves / on any 64 x 64 configuration
        if (tile_count(a, 64, 64) <= 256 && !h2_bare(a)) cfg = g_h2_small_cfg > 0 ? g_h2_small_cfg : 189;
    }
#endif
    return cfg < 0 ? cfg : h2_launch_one(cfg, a, s);
}

// called by emage_gemm_grouped: problems that take the same (groupable) configuration share launches of up to MAXG problems; the rest —
// other configurations, split-K contractions — are launched one by one.  Launch order follows the first problem of each launch.
// count_only: no launch, returns the number of launches the call would make (bench.py's per-launch accounting)
int gemm_h2_dispatch_group(GemmArgs* a, int n, hipStream_t s, bool count_only) {
    int launches = 0;
    int cfg[64];
    bool done[64];
    for (int i = 0; i < n; ++i) {
        cfg[i] = h2_fold_config(a[i], h2_config_for(a[i]));
        if (cfg[i] < 0) return cfg[i];
        done[i] = false;
    }
    // a problem may share a launch when its row has a grouped kernel and it would run neither split-K form alone
    auto groupable = [&](int i) {
        const H2Row* r = h2_row(cfg[i]);
        int per = 0;
        return r && (r->flags & GROUP) && !h2_wants_split_k(a[i], r->t) && !((r->flags & FIXUP) && h2_skf_slices(a[i], &per) >= 2);
    };
    for (int i = 0; i < n; ++i) {
        if (done[i]) continue;
        GemmArgs* grp[MAXG];
        int m = 0;
        if (groupable(i))
            for (int j = i; j < n && m < MAXG; ++j)
                if (!done[j] && cfg[j] == cfg[i] && groupable(j)) { grp[m++] = &a[j]; done[j] = true; }
        int rc;
        ++launches;
        if (count_only) {
            done[i] = true;
            continue;
        }
        if (m >= 2) {
            rc = with_config<H2_CONFIGS>(cfg[i], [&]<H2Row R>() {
                if constexpr (R.flags & GROUP) return launch_h2_group<R.t>(grp, m, s);
                else return (int)EMAGE_EINVAL;
            });
        } else {
            done[i] = true;
            rc = h2_launch_one(cfg[i], a[i], s);
        }
        if (rc) return rc;
    }
    return count_only ? launches : 0;
}

}  // namespace emage_dev