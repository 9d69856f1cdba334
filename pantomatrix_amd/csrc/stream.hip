// Data movement of the streaming batch (pantomatrix_amd/streaming.py): a fixed number of slots, each one live session of
// EmageAudioModel.inference (M:343-470) whose audio arrives while it runs.  Four table-driven kernels, each ONE launch over all slots, so a
// tick is a fixed launch sequence whatever the sessions do — one captured graph:
//   emage_stream_push     scatters the tick's staged PCM into the per-slot audio rings (fp32; s16 decoded x * 2^-15), wrapping at any sample;
//   emage_stream_windows  cuts each ready slot's window out of its ring into a row of the (slots, samples) batch; other rows are zero;
//   emage_stream_commit   appends a ready slot's kept codes to its code ring, takes its new seed rows, and lays out every slot's decode segment;
//   emage_stream_emit     copies each slot's emit range out of the decoded segment and continues its root translation from the carried position.
// All four read the per-tick table (EMAGE_STREAM_WORDS int32 words per slot, emage_hip.h) the host uploads once per tick.  A table row that
// points outside its buffers is skipped (it reads and writes nothing; its outputs are zero) and ORs its bit into the sticky status word.
// Volumes are tiny next to the forward (one window of audio and a few hundred codes per slot): plain element loops, no LDS but the scan's.
// A fifth, emage_stream_push_resample, stands in for emage_stream_push in batches whose sessions push PCM at other rates and layouts: the
// polyphase filter of audio.hip continued across pushes (csrc/pcm_taps.h is shared), driven by a second per-tick table of its own.
// A sixth, emage_stream_push_hints, serves batches whose sessions push MOTION HINTS (keyframes, tracked body parts): it scatters the tick's
// staged hint frames into per-slot hint rings laid out so that every window is 64 contiguous rows, and writes the table
// emage_pack_motion_hints (elementwise.hip) reads them through; driven by a third per-tick table.
#include "common.h"
#include "pcm_taps.h"
#include "rot_math.h"
#include "vel_step.h"

namespace {

constexpr int THREADS = 256;
constexpr int SPANS = 16;                      // blocks per slot of the two audio kernels

struct Row {
    int ready, audio_read, audio_write, push_count, push_src, code_write, seg_read, seg_valid, emit_row, emit_count;
    __device__ explicit Row(const int* t)
        : ready(t[EMAGE_STREAM_READY]), audio_read(t[EMAGE_STREAM_AUDIO_READ]), audio_write(t[EMAGE_STREAM_AUDIO_WRITE]),
          push_count(t[EMAGE_STREAM_PUSH_COUNT]), push_src(t[EMAGE_STREAM_PUSH_SRC]), code_write(t[EMAGE_STREAM_CODE_WRITE]),
          seg_read(t[EMAGE_STREAM_SEG_READ]), seg_valid(t[EMAGE_STREAM_SEG_VALID]), emit_row(t[EMAGE_STREAM_EMIT_ROW]),
          emit_count(t[EMAGE_STREAM_EMIT_COUNT]) {}
};

__device__ __forceinline__ float pcm(const short* p, long i) { return (float)p[i] * (1.f / 32768.f); }
__device__ __forceinline__ float pcm(const float* p, long i) { return p[i]; }

template <typename T>
__global__ __launch_bounds__(THREADS) void push_kernel(const T* __restrict__ staged, long staged_samples, const int* __restrict__ table,
                                                       float* __restrict__ ring, long ring_len, int* __restrict__ status) {
    const Row r(table + (long)blockIdx.x * EMAGE_STREAM_WORDS);
    if (r.push_count == 0) return;
    if (r.push_count < 0 || r.push_count > ring_len || r.push_src < 0 || r.push_src > staged_samples - r.push_count || r.audio_write < 0 ||
        r.audio_write >= ring_len) {
        if (threadIdx.x == 0 && blockIdx.y == 0) atomicOr(status, EMAGE_STREAM_BAD_PUSH);
        return;
    }
    float* o = ring + (long)blockIdx.x * ring_len;
    for (long i = (long)blockIdx.y * THREADS + threadIdx.x; i < r.push_count; i += (long)SPANS * THREADS) {
        long p = r.audio_write + i;
        if (p >= ring_len) p -= ring_len;
        o[p] = pcm(staged, r.push_src + i);
    }
}

// ---- emage_stream_push_resample: the push for PCM at any rate and layout ---------------------------------------------------------------------
// grid (slots, SPANS).  The blocks of a slot share the tiles of EMAGE_AUDIO_TILE outputs of its push as audio.hip's blocks share a clip's: the
// format's phase rows stay in LDS, each tile's input span is decoded into LDS once, and an output is emage_pcm::tap_step over its row in row order — the
// offline kernel's sum, so the bits are the offline kernel's.  A span's frames come from three places: the slot's history (frames before
// this push), the staged PCM, and zeros (before the session's start; behind its end once FINAL).  Block 0 of a slot also writes the slot's
// new history — into the side no block reads in this launch, so there is no order between blocks to keep.
constexpr int TILE = EMAGE_AUDIO_TILE;

struct Format { int pcm, channels, up, down, half, rpp, row_pitch, taps_offset; };      // EMAGE_STREAM_FORMAT_WORDS ints, in the header's order
struct Formats { int n; Format f[EMAGE_STREAM_MAX_FORMATS]; };

struct ResampleRow {
    int frames, src16, format, final, out_count, out_pos, kmax0, r0, hist_valid, hist_side;
    __device__ explicit ResampleRow(const int* t)
        : frames(t[EMAGE_STREAM_RS_FRAMES]), src16(t[EMAGE_STREAM_RS_SRC16]), format(t[EMAGE_STREAM_RS_FORMAT]), final(t[EMAGE_STREAM_RS_FINAL]),
          out_count(t[EMAGE_STREAM_RS_OUT_COUNT]), out_pos(t[EMAGE_STREAM_RS_OUT_POS]), kmax0(t[EMAGE_STREAM_RS_KMAX0]), r0(t[EMAGE_STREAM_RS_R0]),
          hist_valid(t[EMAGE_STREAM_RS_HIST_VALID]), hist_side(t[EMAGE_STREAM_RS_HIST_SIDE]) {}
};

// frame k of the session, counted from the first staged one, as mono fp32: k < 0 lies in the history (hist[hist_len - 1] is frame -1)
template <int FMT> __device__ __forceinline__ float stream_frame(long k, const unsigned char* src, int frames, int channels, const float* hist,
                                                                 int hist_len, int hist_valid) {
    if (k >= 0) return k < frames ? emage_pcm::decode_frame<FMT>(src + k * (channels * emage_pcm::sample_bytes(FMT)), channels) : 0.f;
    return k >= -(long)hist_valid ? hist[hist_len + k] : 0.f;
}

template <int FMT> __device__ __forceinline__ void resample_slot(const ResampleRow& r, const Format& f, const unsigned char* src, const float* __restrict__ taps,
                                                                 float* __restrict__ ring, long ring_len, float* hist, int hist_len, float* smem) {
    const int tid = threadIdx.x;
    const float* h_old = hist + (long)r.hist_side * hist_len;
    if (blockIdx.y == 0 && r.frames > 0) {               // the last hist_len frames of (old history ++ push): entry hist_len - j is frame -j of the NEXT push
        float* h_new = hist + (long)(1 - r.hist_side) * hist_len;
        for (int j = tid + 1; j <= hist_len; j += THREADS) h_new[hist_len - j] = stream_frame<FMT>((long)r.frames - j, src, r.frames, f.channels, h_old, hist_len, r.hist_valid);
    }
    const int n_tiles = (r.out_count + TILE - 1) / TILE;
    if ((int)blockIdx.y >= n_tiles) return;
    const bool filter = f.up != f.down;                   // up == down == 1: decode and channel mean only, as audio_decode_kernel
    const int table = filter ? f.up * f.row_pitch : 0;
    float* s_h = smem;                                    // up rows of row_pitch taps
    float* s_x = smem + ((table + 3) & ~3);               // the tile's decoded span
    const float* rows = taps + f.taps_offset;             // 16-byte aligned: the offset is a multiple of 4 floats
    for (int i = tid; i < table / 4; i += THREADS) ((float4*)s_h)[i] = ((const float4*)rows)[i];
    for (int i = (table & ~3) + tid; i < table; i += THREADS) s_h[i] = rows[i];
    for (int tile = blockIdx.y; tile < n_tiles; tile += gridDim.y) {
        const int j0 = tile * TILE;                       // outputs are counted from the push's first, m0: nothing here is an absolute position
        const int n = r.out_count - j0 < TILE ? r.out_count - j0 : TILE;
        const long base0 = (long)j0 * f.down + r.r0;      // (m down + half) - (the first output's kmax) up, in 64 bits as audio.hip's base0
        const long q0 = r.kmax0 + base0 / f.up;           // newest frame the tile's first output reads
        const int rt = (int)(base0 % f.up);
        const long k0 = q0 - (f.rpp - 1);                 // oldest frame any output of the tile reads
        const int count = (int)(((long)(n - 1) * f.down + rt) / f.up) + f.rpp;
        __syncthreads();                                  // the previous tile's readers are done with s_x
        for (int i = tid; i < count; i += THREADS) s_x[i] = stream_frame<FMT>(k0 + i, src, r.frames, f.channels, h_old, hist_len, r.hist_valid);
        __syncthreads();
        for (int o = tid; o < n; o += THREADS) {
            const int d = o * f.down + rt;                // fits 32 bits: TILE * down + up < 2^31 for up, down <= 65536
            const float* x = s_x + (f.rpp - 1) + d / f.up;
            long p = (long)r.out_pos + j0 + o;
            if (p >= ring_len) p -= ring_len;
            float acc = x[0];
            if (filter) {
                const float* h = s_h + (d % f.up) * f.row_pitch;
                acc = 0.f;
                for (int i = 0; i < f.rpp; ++i) acc = emage_pcm::tap_step(acc, h, x, i);
            }
            ring[p] = acc;
        }
    }
}

__global__ __launch_bounds__(THREADS) void push_resample_kernel(const unsigned char* __restrict__ staged, long staged_bytes, const int* __restrict__ rs_table,
                                                                Formats fmts, const float* __restrict__ taps, float* __restrict__ ring, long ring_len,
                                                                float* history, int hist_len, int* __restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) float s_resample[];
    const ResampleRow r(rs_table + (long)blockIdx.x * EMAGE_STREAM_RS_WORDS);
    if (r.frames == 0 && r.out_count == 0) return;
    const bool known = r.format >= 0 && r.format < fmts.n;
    const Format f = fmts.f[known ? r.format : 0];
    bool ok = known && r.frames >= 0 && r.src16 >= 0 && r.out_count >= 0 && r.out_count <= ring_len && r.out_pos >= 0 && r.out_pos < ring_len &&
              r.kmax0 >= 0 && r.r0 >= 0 && r.r0 < f.up && r.hist_valid >= 0 && r.hist_valid <= hist_len && (r.hist_side == 0 || r.hist_side == 1) &&
              (long)r.src16 * 16 + (long)r.frames * (f.channels * emage_pcm::sample_bytes(f.pcm)) <= staged_bytes;
    // without FINAL every frame an output reads must exist: the newest one the last output reads lies inside the staged frames
    if (ok && !r.final && r.out_count > 0) ok = r.kmax0 + ((long)(r.out_count - 1) * f.down + r.r0) / f.up < r.frames;
    if (!ok) {
        if (threadIdx.x == 0 && blockIdx.y == 0) atomicOr(status, EMAGE_STREAM_BAD_RESAMPLE);
        return;
    }
    const unsigned char* src = staged + (long)r.src16 * 16;
    float* o = ring + (long)blockIdx.x * ring_len;
    float* hist = history + (long)blockIdx.x * 2 * hist_len;
    if (f.pcm == EMAGE_PCM_S16) resample_slot<EMAGE_PCM_S16>(r, f, src, taps, o, ring_len, hist, hist_len, s_resample);
    else if (f.pcm == EMAGE_PCM_S24) resample_slot<EMAGE_PCM_S24>(r, f, src, taps, o, ring_len, hist, hist_len, s_resample);
    else if (f.pcm == EMAGE_PCM_S32) resample_slot<EMAGE_PCM_S32>(r, f, src, taps, o, ring_len, hist, hist_len, s_resample);
    else resample_slot<EMAGE_PCM_F32>(r, f, src, taps, o, ring_len, hist, hist_len, s_resample);
}

// ---- emage_stream_push_hints: the tick's motion hints into the hint rings, and the windows' table -------------------------------------------
// grid (slots, HINT_SPANS).  Frame f of a session lives at ring row f mod hint_rows; rows hint_rows .. hint_rows + 3 mirror rows 0 .. 3, so a
// frame that lands below row 4 is written twice and window i is the 64 contiguous rows from (60 i) mod hint_rows.  A slot's chunk of the
// staged buffer is COUNT rows of W floats and then COUNT rows of HINT_C mask bytes.  Every block of a slot evaluates the same checks; block 0
// writes the slot's row of the window table.  Volumes: at most hint_rows x 344 x 5 bytes per slot — latency, not bandwidth.
constexpr int HINT_SPANS = 8;
constexpr int HINT_C = 337, HINT_JOINTS = 55, HINT_PRE = 4, HINT_TRACKER_W = 172;     // 55 x rot6d | 3 | 4;  55 x axis-angle | 3 | 4

struct HintPush {
    int count, src16, form, write, seed_row, seed_count, ready, win_first, win_avail;
    __device__ explicit HintPush(const int* t)
        : count(t[EMAGE_STREAM_HINT_COUNT]), src16(t[EMAGE_STREAM_HINT_SRC16]), form(t[EMAGE_STREAM_HINT_FORM]), write(t[EMAGE_STREAM_HINT_WRITE]),
          seed_row(t[EMAGE_STREAM_HINT_SEED_ROW]), seed_count(t[EMAGE_STREAM_HINT_SEED_COUNT]), ready(t[EMAGE_STREAM_HINT_READY]),
          win_first(t[EMAGE_STREAM_HINT_WIN_FIRST]), win_avail(t[EMAGE_STREAM_HINT_WIN_AVAIL]) {}
};

__global__ __launch_bounds__(THREADS) void push_hints_kernel(const unsigned char* __restrict__ staged, long staged_bytes, const int* __restrict__ hint_table,
                                                             float* __restrict__ ring_motion, unsigned char* __restrict__ ring_keep, int hint_rows, int ld,
                                                             float* __restrict__ seeds, long long* __restrict__ window_table, int window,
                                                             int* __restrict__ status) {
    const int s = blockIdx.x, tid = threadIdx.x;
    const HintPush r(hint_table + (long)s * EMAGE_STREAM_HINT_WORDS);
    const bool tracker = r.form == EMAGE_STREAM_HINT_TRACKER;
    const int w = tracker ? HINT_TRACKER_W : HINT_C;
    bool ok = r.count >= 0 && r.count <= hint_rows && r.src16 >= 0 && (r.form == EMAGE_STREAM_HINT_PACKED || tracker) && r.write >= 0 &&
              r.write < hint_rows && (long)r.src16 * 16 + (long)r.count * (w * 4 + HINT_C) <= staged_bytes;
    if (ok && r.seed_count != 0)
        ok = r.seed_count > 0 && r.seed_row == r.write && r.seed_row + r.seed_count <= HINT_PRE && r.seed_count <= r.count;
    if (ok && r.ready) ok = r.win_avail >= 0 && r.win_avail <= window && r.win_first >= 0 && r.win_first + window <= hint_rows + HINT_PRE;
    const long rows = hint_rows + HINT_PRE;                // the slot's rows of the two planes
    if (blockIdx.y == 0 && tid == 0) {
        const bool hinted = ok && r.ready;
        window_table[2 * (long)s] = hinted ? (long long)s * rows + r.win_first : 0;
        window_table[2 * (long)s + 1] = hinted ? r.win_avail : 0;
        if (!ok) atomicOr(status, EMAGE_STREAM_BAD_HINTS);
    }
    if (!ok || r.count == 0) return;
    const float* src = (const float*)(staged + (long)r.src16 * 16);
    const unsigned char* mask = (const unsigned char*)(src + (long)r.count * w);
    float* om = ring_motion + (long)s * rows * ld;
    unsigned char* okeep = ring_keep + (long)s * rows * ld;
    float* seed = seeds + ((long)s * HINT_PRE + r.seed_row) * HINT_C;
    const int first = blockIdx.y * THREADS + tid, stride = HINT_SPANS * THREADS;
    // the keep plane, the padding columns, and the motion columns that are copied (all of them in the packed form, 330 .. 336 in the tracker's)
    for (int i = first; i < r.count * ld; i += stride) {
        const int j = i / ld, c = i - j * ld;
        int p = r.write + j;
        if (p >= hint_rows) p -= hint_rows;
        const unsigned char k = c < HINT_C ? mask[(long)j * HINT_C + c] : (unsigned char)1;
        okeep[(long)p * ld + c] = k;
        if (p < HINT_PRE) okeep[(long)(hint_rows + p) * ld + c] = k;
        if (tracker && c < 6 * HINT_JOINTS) continue;
        const float v = c >= HINT_C ? 0.f : tracker ? src[(long)j * HINT_TRACKER_W + c - 6 * HINT_JOINTS + 3 * HINT_JOINTS] : src[(long)j * HINT_C + c];
        om[(long)p * ld + c] = v;
        if (p < HINT_PRE) om[(long)(hint_rows + p) * ld + c] = v;
        if (j < r.seed_count && c < HINT_C) seed[(long)j * HINT_C + c] = v;
    }
    if (!tracker) return;
    for (int i = first; i < r.count * HINT_JOINTS; i += stride) {                 // one joint per thread: emage_axis_angle_to_rot6d's bits
        const int j = i / HINT_JOINTS, q = i - j * HINT_JOINTS;
        int p = r.write + j;
        if (p >= hint_rows) p -= hint_rows;
        float aa[3], d6[6];
        for (int c = 0; c < 3; ++c) aa[c] = src[(long)j * HINT_TRACKER_W + q * 3 + c];
        emage_rot::aa_to_rot6d(aa, d6);
        for (int c = 0; c < 6; ++c) {
            om[(long)p * ld + q * 6 + c] = d6[c];
            if (p < HINT_PRE) om[(long)(hint_rows + p) * ld + q * 6 + c] = d6[c];
            if (j < r.seed_count) seed[(long)j * HINT_C + q * 6 + c] = d6[c];
        }
    }
}

__global__ __launch_bounds__(THREADS) void windows_kernel(const float* __restrict__ ring, long ring_len, const int* __restrict__ table, int samples,
                                                          float* __restrict__ out, long ld, int* __restrict__ status) {
    const Row r(table + (long)blockIdx.x * EMAGE_STREAM_WORDS);
    float* o = out + (long)blockIdx.x * ld;
    bool ok = r.ready != 0;
    if (ok && (r.audio_read < 0 || r.audio_read >= ring_len)) {
        if (threadIdx.x == 0 && blockIdx.y == 0) atomicOr(status, EMAGE_STREAM_BAD_WINDOW);
        ok = false;
    }
    const float* src = ring + (long)blockIdx.x * ring_len;
    for (int i = blockIdx.y * THREADS + threadIdx.x; i < samples; i += SPANS * THREADS) {
        long p = (long)r.audio_read + i;
        if (p >= ring_len) p -= ring_len;
        o[i] = ok ? src[p] : 0.f;
    }
}

// block = one slot.  Phase 1 (ready slots): codes and seed rows into the slot's state; phase 2 (every slot): the decode segment out of the
// code ring, rows beyond seg_valid — and every row of a slot that is not ready — code 0.
__global__ __launch_bounds__(THREADS) void commit_kernel(const int* __restrict__ table, int parts, const int64_t* __restrict__ win_codes, int window,
                                                         int keep, int64_t* __restrict__ code_ring, int ring_codes, int64_t* __restrict__ segment,
                                                         int seg_len, const float* __restrict__ new_seed, long ld_seed, float* __restrict__ seeds,
                                                         int seed_floats, int slots, int* __restrict__ status) {
    const int s = blockIdx.x, tid = threadIdx.x;
    const Row r(table + (long)s * EMAGE_STREAM_WORDS);
    bool ok = r.ready != 0;
    if (ok && (r.code_write < 0 || r.code_write >= ring_codes || r.seg_read < 0 || r.seg_read >= ring_codes || r.seg_valid < 0 ||
               r.seg_valid > seg_len || r.seg_valid > ring_codes)) {
        if (tid == 0) atomicOr(status, EMAGE_STREAM_BAD_COMMIT);
        ok = false;
    }
    if (ok) {
        for (int i = tid; i < parts * keep; i += THREADS) {
            const int p = i / keep, j = i - p * keep;
            int c = r.code_write + j;
            if (c >= ring_codes) c -= ring_codes;
            code_ring[((long)p * slots + s) * ring_codes + c] = win_codes[((long)p * slots + s) * window + j];
        }
        for (int i = tid; i < seed_floats; i += THREADS) seeds[(long)s * seed_floats + i] = new_seed[(long)s * ld_seed + i];
    }
    __syncthreads();                                                   // the segment reads the codes this block has just appended
    for (int i = tid; i < parts * seg_len; i += THREADS) {
        const int p = i / seg_len, j = i - p * seg_len;
        int64_t v = 0;
        if (ok && j < r.seg_valid) {
            int c = r.seg_read + j;
            if (c >= ring_codes) c -= ring_codes;
            v = code_ring[((long)p * slots + s) * ring_codes + c];
        }
        segment[((long)p * slots + s) * seg_len + j] = v;
    }
}

// block = one slot: rows [emit_row, emit_row + emit_count) of the decoded segment into rows [0, emit_count) of the outputs, zeros behind.
__global__ __launch_bounds__(THREADS) void emit_kernel(const int* __restrict__ table, int seg_len, int out_rows, const float* __restrict__ aa,
                                                       const float* __restrict__ expr, const float* __restrict__ vel, int ldv, int col0, float dt,
                                                       const int64_t* __restrict__ segment, int parts, int slots, float* __restrict__ carry,
                                                       float* __restrict__ poses, float* __restrict__ expressions, float* __restrict__ trans,
                                                       int64_t* __restrict__ codes, int* __restrict__ status) {
    extern __shared__ float s_v[];                                     // [3][count]: the emitted rows' velocity columns, then the positions
    const int s = blockIdx.x, tid = threadIdx.x;
    const Row r(table + (long)s * EMAGE_STREAM_WORDS);
    int n = r.ready ? r.emit_count : 0;
    if (r.ready && (n < 0 || n > out_rows || r.emit_row < 0 || r.emit_row > seg_len - n)) {
        if (tid == 0) atomicOr(status, EMAGE_STREAM_BAD_EMIT);
        n = 0;
    }
    const long row0 = (long)s * seg_len + r.emit_row, out0 = (long)s * out_rows;
    for (int i = tid; i < out_rows * 165; i += THREADS) poses[out0 * 165 + i] = i < n * 165 ? aa[row0 * 165 + i] : 0.f;
    for (int i = tid; i < out_rows * 100; i += THREADS) expressions[out0 * 100 + i] = i < n * 100 ? expr[row0 * 100 + i] : 0.f;
    for (int i = tid; i < out_rows * parts; i += THREADS) {
        const int j = i / parts, p = i - j * parts;
        codes[out0 * parts + i] = j < n ? segment[((long)p * slots + s) * seg_len + r.emit_row + j] : 0;
    }
    for (int i = tid; i < 3 * n; i += THREADS) {
        const int t = i / 3, ax = i - t * 3;
        s_v[ax * n + t] = vel[(row0 + t) * ldv + col0 + ax];
    }
    __syncthreads();
    if (tid < 2 && n > 0) {                                            // x (axis 0) and z (axis 2) integrate; row t holds the position AT frame t
        const int ax = tid * 2;
        float pos = carry[(long)s * 3 + ax];
        float* p = s_v + ax * n;
        for (int t = 0; t < n; ++t) {
            const float v = p[t];
            p[t] = pos;
            pos = emage_vel::step(pos, v, dt);
        }
        carry[(long)s * 3 + ax] = pos;                                 // the position of the first frame not emitted yet
    }
    __syncthreads();
    for (int i = tid; i < out_rows * 3; i += THREADS) {
        const int t = i / 3, ax = i - t * 3;
        trans[out0 * 3 + i] = t < n ? s_v[ax * n + t] : 0.f;           // y (axis 1) is the decoded height, copied through
    }
}

}  // namespace

extern "C" int emage_stream_push(int audio_fmt, const void* staged, long staged_samples, const int* table, int slots, float* ring, long ring_len,
                                 int* status, void* stream) {
    if (!staged || !table || !ring || !status) return EMAGE_EINVAL;
    if (audio_fmt != EMAGE_PCM_S16 && audio_fmt != EMAGE_PCM_F32) return EMAGE_EINVAL;
    if (slots <= 0 || staged_samples <= 0 || ring_len <= 0 || ring_len > 0x7fffffffL || staged_samples > 0x7fffffffL) return EMAGE_EINVAL;
    if (((uintptr_t)staged & (audio_fmt == EMAGE_PCM_S16 ? 1 : 3)) || ((uintptr_t)table & 3) || ((uintptr_t)ring & 3) || ((uintptr_t)status & 3)) return EMAGE_EINVAL;
    if (audio_fmt == EMAGE_PCM_S16)
        hipLaunchKernelGGL(push_kernel<short>, dim3((unsigned)slots, SPANS), dim3(THREADS), 0, (hipStream_t)stream, (const short*)staged, staged_samples,
                           table, ring, ring_len, status);
    else
        hipLaunchKernelGGL(push_kernel<float>, dim3((unsigned)slots, SPANS), dim3(THREADS), 0, (hipStream_t)stream, (const float*)staged, staged_samples,
                           table, ring, ring_len, status);
    return launch_status();
}

extern "C" int emage_stream_push_resample(const void* staged, long staged_bytes, const int* rs_table, int slots, const int* formats, int n_formats,
                                          const float* taps, long taps_floats, float* ring, long ring_len, float* history, int hist_len, int* status,
                                          void* stream) {
    if (!staged || !rs_table || !formats || !taps || !ring || !history || !status) return EMAGE_EINVAL;
    if (slots <= 0 || slots > 65535 || staged_bytes <= 0 || taps_floats <= 0 || ring_len <= 0 || ring_len > 0x7fffffffL || hist_len <= 0) return EMAGE_EINVAL;
    if (n_formats <= 0 || n_formats > EMAGE_STREAM_MAX_FORMATS) return EMAGE_EINVAL;
    if ((((uintptr_t)staged | (uintptr_t)taps) & 15) || (((uintptr_t)rs_table | (uintptr_t)ring | (uintptr_t)history | (uintptr_t)status) & 3)) return EMAGE_EINVAL;
    Formats fmts{};
    fmts.n = n_formats;
    long lds_floats = 0;
    for (int i = 0; i < n_formats; ++i) {
        const int* w = formats + (long)i * EMAGE_STREAM_FORMAT_WORDS;
        const Format f{w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7]};
        if (f.pcm < EMAGE_PCM_S16 || f.pcm > EMAGE_PCM_F32 || f.channels < 1 || f.channels > 8) return EMAGE_EINVAL;
        if (f.up <= 0 || f.down <= 0 || f.up > (1 << 16) || f.down > (1 << 16) || (f.up == f.down && f.up != 1)) return EMAGE_EINVAL;
        long table = 0;
        if (f.up == f.down) {
            if (f.half != 0 || f.rpp != 1 || f.row_pitch != 0 || f.taps_offset != 0) return EMAGE_EINVAL;
        } else {                                          // the geometry emage_audio_resample derives from (up, down), and its two LDS budgets
            const int half = 10 * (f.up > f.down ? f.up : f.down), rpp = (2 * half + f.up) / f.up;
            table = (long)f.up * (rpp | 1);
            if (f.half != half || f.rpp != rpp || f.row_pitch != (rpp | 1)) return EMAGE_EINVAL;
            if (f.taps_offset < 0 || (f.taps_offset & 3) || f.taps_offset + table > taps_floats || table * 4 > EMAGE_AUDIO_TAPS_LDS_BYTES) return EMAGE_EINVAL;
        }
        const long span_cap = ((long)(TILE - 1) * f.down + f.up - 1) / f.up + f.rpp + 1 + emage_pcm::SPAN_SLACK;
        if (span_cap * 4 > EMAGE_AUDIO_SPAN_LDS_BYTES || f.rpp - 1 > hist_len) return EMAGE_EINVAL;
        const long need = ((table + 3) & ~3L) + span_cap;
        if (need > lds_floats) lds_floats = need;
        fmts.f[i] = f;
    }
    static const hipError_t configured = hipFuncSetAttribute((const void*)push_resample_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (configured != hipSuccess) return (int)configured;
    hipLaunchKernelGGL(push_resample_kernel, dim3((unsigned)slots, SPANS), dim3(THREADS), (size_t)lds_floats * sizeof(float), (hipStream_t)stream,
                       (const unsigned char*)staged, staged_bytes, rs_table, fmts, taps, ring, ring_len, history, hist_len, status);
    return launch_status();
}

extern "C" int emage_stream_push_hints(const void* staged, long staged_bytes, const int* hint_table, int slots, float* ring_motion, unsigned char* ring_keep,
                                       int hint_rows, int ld, float* seeds, long long* window_table, int window, int* status, void* stream) {
    if (!staged || !hint_table || !ring_motion || !ring_keep || !seeds || !window_table || !status) return EMAGE_EINVAL;
    if (slots <= 0 || slots > 65535 || staged_bytes <= 0 || hint_rows < 120 || hint_rows % 60 || hint_rows > (1 << 16) || ld < HINT_C || ld > 4096 || window <= 0 ||
        window > hint_rows)
        return EMAGE_EINVAL;
    if (((uintptr_t)staged & 15) || (((uintptr_t)hint_table | (uintptr_t)ring_motion | (uintptr_t)seeds | (uintptr_t)status) & 3) || ((uintptr_t)window_table & 7))
        return EMAGE_EINVAL;
    hipLaunchKernelGGL(push_hints_kernel, dim3((unsigned)slots, HINT_SPANS), dim3(THREADS), 0, (hipStream_t)stream, (const unsigned char*)staged,
                       staged_bytes, hint_table, ring_motion, ring_keep, hint_rows, ld, seeds, window_table, window, status);
    return launch_status();
}

extern "C" int emage_stream_windows(const float* ring, long ring_len, const int* table, int slots, int samples, float* out, long ld_out,
                                    int* status, void* stream) {
    if (!ring || !table || !out || !status) return EMAGE_EINVAL;
    if (slots <= 0 || samples <= 0 || ring_len <= 0 || ring_len > 0x7fffffffL || samples > ring_len || ld_out < samples) return EMAGE_EINVAL;
    if (((uintptr_t)ring & 3) || ((uintptr_t)table & 3) || ((uintptr_t)out & 3) || ((uintptr_t)status & 3)) return EMAGE_EINVAL;
    hipLaunchKernelGGL(windows_kernel, dim3((unsigned)slots, SPANS), dim3(THREADS), 0, (hipStream_t)stream, ring, ring_len, table, samples, out, ld_out,
                       status);
    return launch_status();
}

extern "C" int emage_stream_commit(const int* table, int slots, int parts, const int64_t* win_codes, int window, int keep, int64_t* code_ring,
                                   int ring_codes, int64_t* segment, int seg_len, const float* new_seed, long ld_seed, float* seeds, int seed_floats,
                                   int* status, void* stream) {
    if (!table || !win_codes || !code_ring || !segment || !new_seed || !seeds || !status) return EMAGE_EINVAL;
    if (slots <= 0 || parts <= 0 || parts > 4 || window <= 0 || keep <= 0 || keep > window || ring_codes < keep || seg_len <= 0 || seed_floats <= 0 ||
        ld_seed < seed_floats)
        return EMAGE_EINVAL;
    if (((uintptr_t)table & 3) || ((uintptr_t)win_codes & 7) || ((uintptr_t)code_ring & 7) || ((uintptr_t)segment & 7) || ((uintptr_t)new_seed & 3) ||
        ((uintptr_t)seeds & 3) || ((uintptr_t)status & 3))
        return EMAGE_EINVAL;
    hipLaunchKernelGGL(commit_kernel, dim3((unsigned)slots), dim3(THREADS), 0, (hipStream_t)stream, table, parts, win_codes, window, keep, code_ring,
                       ring_codes, segment, seg_len, new_seed, ld_seed, seeds, seed_floats, slots, status);
    return launch_status();
}

extern "C" int emage_stream_emit(const int* table, int slots, int seg_len, int out_rows, const float* axis_angle, const float* expression,
                                 const float* vel, int ldv, int col0, float dt, const int64_t* segment, int parts, float* carry, float* poses,
                                 float* expressions, float* trans, int64_t* codes, int* status, void* stream) {
    if (!table || !axis_angle || !expression || !vel || !segment || !carry || !poses || !expressions || !trans || !codes || !status) return EMAGE_EINVAL;
    if (slots <= 0 || seg_len <= 0 || out_rows <= 0 || out_rows > 4096 || parts <= 0 || parts > 4 || col0 < 0 || ldv < col0 + 3) return EMAGE_EINVAL;
    if (((uintptr_t)table & 3) || ((uintptr_t)segment & 7) || ((uintptr_t)codes & 7) || ((uintptr_t)status & 3)) return EMAGE_EINVAL;
    hipLaunchKernelGGL(emit_kernel, dim3((unsigned)slots), dim3(THREADS), (size_t)3 * out_rows * sizeof(float), (hipStream_t)stream, table, seg_len,
                       out_rows, axis_angle, expression, vel, ldv, col0, dt, segment, parts, slots, carry, poses, expressions, trans, codes, status);
    return launch_status();
}
