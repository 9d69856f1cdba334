// emage_gemm, EMAGE_H2 mode, ANTIPHASE tile configurations (h2_pp_tile.h; round 6): one 8-wave block per CU whose two wave groups run
// the K-loop half a step apart on ONE shared A / W panel.  Dispatched by gemm_h2.hip (configuration ids 300-399).
#include "common.h"
#include <utility>
#include "h2_pp_tile.h"

#ifdef EMAGE_TOOLS       // every antiphase configuration is the tools build's
namespace emage_dev {
extern unsigned long long* g_h2_trace;
}

namespace {

using namespace emage_dev;

// One antiphase tile configuration: the template arguments of gemm_h2_pp_tile, by name
struct PpTile {
    int bm, bn;                  // block tile
    int wm = 4, wn = 2;          // wave grid
    int ns = 4;                  // ring depth in K-tiles
    bool prio = true;            // s_setprio around the MFMA clusters
    bool trace = false;          // phase tracer
    int mode = 0;                // where the DMA pieces are issued (1: in front of the fragment reads; 2: between the MFMAs of the C phase)
};
struct PpRow {
    int id;
    PpTile t;
    bool group = false;          // has a grouped kernel (emage_gemm_grouped)
};
// THE antiphase configurations; every launcher and kernel below takes its row from here
constexpr PpRow PP_CONFIGS[] = {
    // round 6 (VERDICT next #1b): ANTIPHASE tiles — one 8-wave block per CU, two wave groups half a K-step apart (h2_pp_tile.h)
    {300, {.bm = 128, .bn = 96}, true},                                       // 768-wide: 256 tiles of 128 x 96 at M = 4096; waves 32 x 48
    {301, {.bm = 128, .bn = 96, .prio = false}, true},                        // ... without s_setprio around the MFMA clusters
    {302, {.bm = 128, .bn = 96, .ns = 3}, true},                              // ring of 3
    {303, {.bm = 128, .bn = 96, .ns = 5}, true},                              // ring of 5 (140 KB)
    {310, {.bm = 128, .bn = 192, .ns = 3}},                                   // 1536- / 2304-wide: waves 32 x 96
    {311, {.bm = 128, .bn = 192, .wm = 2, .wn = 4, .ns = 3}},                 // waves 64 x 48
    {312, {.bm = 128, .bn = 192, .wm = 2, .wn = 4}},                          // ring of 4 (160 KB)
    {320, {.bm = 64, .bn = 192, .wm = 2, .wn = 4}},                           // 64 x 192: waves 32 x 48
    {321, {.bm = 64, .bn = 192, .wm = 2, .wn = 4, .ns = 5}},
    {330, {.bm = 64, .bn = 64, .wm = 2, .wn = 4, .ns = 6}},                   // the N = 256 heads: one 64 x 64 tile per CU, waves 32 x 16
    {331, {.bm = 128, .bn = 64, .ns = 5}},                                    // waves 32 x 32
    {350, {.bm = 128, .bn = 96, .trace = true}},                              // 300 with the phase tracer
    // v2: where the DMA pieces are issued (MODE 1: in front of the fragment reads; MODE 2: between the MFMAs of the C phase)
    {340, {.bm = 128, .bn = 96, .mode = 1}},
    {341, {.bm = 128, .bn = 96, .mode = 2}},
    {342, {.bm = 128, .bn = 96, .ns = 5, .mode = 2}},
    {343, {.bm = 128, .bn = 96, .ns = 5, .prio = false, .mode = 2}},
    {344, {.bm = 64, .bn = 192, .wm = 2, .wn = 4, .ns = 5, .mode = 2}},
    {345, {.bm = 128, .bn = 192, .wm = 2, .wn = 4, .mode = 2}},
    {346, {.bm = 128, .bn = 192, .mode = 2}},
    {351, {.bm = 128, .bn = 96, .trace = true, .mode = 1}},                   // tracers
    {352, {.bm = 128, .bn = 96, .ns = 5, .trace = true, .mode = 2}},
};
static_assert(unique_config_ids<PP_CONFIGS>(), "one row per id");
constexpr bool pp_rows_consistent() {
    for (const PpRow& r : PP_CONFIGS) if (r.group && (r.t.trace || r.t.mode != 0)) return false;     // what gemm_h2_pp_group_kernel runs
    return true;
}
static_assert(pp_rows_consistent(), "a grouped row the grouped kernel cannot run");

template <PpTile C>
__global__ __launch_bounds__(512, 2) void gemm_h2_pp_kernel(GemmArgs p) {
    __shared__ __attribute__((aligned(128))) unsigned char smem[h2_pp_smem_bytes<C.bm, C.bn, C.ns>()];
    const int nblk = p.tiles_m * p.tiles_n;
    int bid = (int)blockIdx.x;
    if (p.tile_order == 0 && !EMAGE_DBG(p, 32)) bid = xcd_run_order(bid, nblk);
    const int tile_n = bid % p.tiles_n, tile_m = bid / p.tiles_n;
    gemm_h2_pp_tile<C.bm, C.bn, C.wm, C.wn, C.ns, C.prio, C.trace, C.mode>(p, tile_m * C.bm, tile_n * C.bn, smem);
}

template <PpTile C>
int launch_h2_pp(GemmArgs& a, hipStream_t s) {
    if (a.out_t && a.t_col0 % C.bn != 0) return EMAGE_EINVAL;      // a tile is either row-major or transposed
    if (a.ln_stats || a.rs_stats || a.st_out) return EMAGE_EINVAL; // no LayerNorm fold in these tiles
    set_tile_grid(a, C.bm, C.bn);
    a.trace = C.trace ? g_h2_trace : nullptr;
    a.tile_order = 0;
    a.ksplit = 1;
    a.ws = nullptr; a.ws_plane = 0; a.ldws = 0;
    hipLaunchKernelGGL((gemm_h2_pp_kernel<C>), dim3(a.tiles_m * a.tiles_n), dim3(512), 0, s, a);
    return launch_status();
}

// grouped launch (gemm_h2.hip `launch_h2_group`): the problems' tiles concatenated, XCD-aware order over the whole grid
template <PpTile C>
__global__ __launch_bounds__(512, 2) void gemm_h2_pp_group_kernel(GroupArgs g) {
    __shared__ __attribute__((aligned(128))) unsigned char smem[h2_pp_smem_bytes<C.bm, C.bn, C.ns>()];
    const int bid = xcd_run_order((int)blockIdx.x, g.total);
    int pi = 0;
#pragma unroll
    for (int i = 0; i < MAXG - 1; ++i) pi += (i + 1 < g.n && bid >= g.tile_end[i]) ? 1 : 0;
    pi = __builtin_amdgcn_readfirstlane(pi);
    const int t = bid - (pi ? g.tile_end[pi - 1] : 0);
    const GemmArgs& p = g.p[pi];
    const int tile_n = t % p.tiles_n, tile_m = t / p.tiles_n;
    gemm_h2_pp_tile<C.bm, C.bn, C.wm, C.wn, C.ns, C.prio, C.trace, C.mode>(p, tile_m * C.bm, tile_n * C.bn, smem);
}

template <PpTile C>
int launch_h2_pp_group(GemmArgs** a, int n, hipStream_t s) {
    GroupArgs g;
    const int rc = fill_group(g, a, n, C.bm, C.bn);
    if (rc) return rc;
    hipLaunchKernelGGL((gemm_h2_pp_group_kernel<C>), dim3(g.total), dim3(512), 0, s, g);
    return launch_status();
}

}  // namespace

namespace emage_dev {

__attribute__((visibility("hidden"))) bool pp_groupable(int cfg) {
    for (const PpRow& r : PP_CONFIGS) if (r.id == cfg) return r.group;
    return false;
}

int run_pp_group(int cfg, GemmArgs** a, int n, hipStream_t s) {
    return with_config<PP_CONFIGS>(cfg, [&]<PpRow R>() {
        if constexpr (R.group) return launch_h2_pp_group<R.t>(a, n, s);
        else return (int)EMAGE_EINVAL;
    });
}

int run_pp_config(int cfg, GemmArgs& a, hipStream_t s) {
    return with_config<PP_CONFIGS>(cfg, [&]<PpRow R>() { return launch_h2_pp<R.t>(a, s); });
}

}  // namespace emage_dev

#else       // the product library: no such configuration

namespace emage_dev {
__attribute__((visibility("hidden"))) bool pp_groupable(int) { return false; }
int run_pp_group(int, GemmArgs**, int, hipStream_t) { return EMAGE_EINVAL; }
int run_pp_config(int, GemmArgs&, hipStream_t) { return EMAGE_EINVAL; }
}

#endif
