// emage_audio_resample — the audio front end in one launch: interleaved PCM (16 / 24 / 32-bit integer or float32, 1..8 channels, any
// rate) -> mono float32 at the model's rate.  Per output sample: decode, channel mean, rational-rate polyphase low-pass
//   y[m] = sum_k h[m*down + half - k*up] * x[k]        (what scipy.signal.resample_poly(x, up, down) computes, in fp32)
// A block owns tiles of EMAGE_AUDIO_TILE outputs of one clip.  Per tile it decodes and down-mixes the tile's input span (tile + the
// filter's reach) into LDS once; the phase rows of the filter stay in LDS for all of the block's tiles.  Output m uses phase row
// p = (m*down + half) mod up from its first entry, against x[kmax], x[kmax - 1], ... with kmax = (m*down + half) / up.  Rows are padded
// with zeros to a common ODD pitch.  The tap loop reads one float per lane (ds_read_b32: 32 banks, lanes 0-31 and 32-63 served apart): lane l of a
// group reads row (r0 + l*down) mod up at bank (row*pitch + i) mod 32, and an odd pitch makes row -> row*pitch a bijection mod 32.  Where 32 divides
// up (160, 320, 640) the rows of 32 neighbouring lanes are r0 + l*down mod 32, all different when down is odd (441): conflict-free; up = 1 is a
// broadcast, up = 2 two addresses.  The x reads are NOT conflict-free when down > up: lanes step floor(l*down/up) frames (2.76 at 44.1 kHz), so
// 32 lanes span ~88 words of 32 banks, about 3 lanes per bank.  Samples outside [0, n_in) are zeros in the LDS span, so the tap loop has no bounds tests.
// Every output has one writer and a fixed summation order (taps in row order): the result is bit-reproducible.
#include "common.h"
#include "pcm_taps.h"

namespace {

using emage_pcm::decode_frame;                // the decode, the channel mean and the tap walk are the streaming resampler's too (stream.hip)
using emage_pcm::sample_bytes;

constexpr int TILE = EMAGE_AUDIO_TILE;
constexpr int THREADS = 256;
constexpr int SPAN_SLACK = emage_pcm::SPAN_SLACK;    // the vector-load path starts its span on a 16-byte chunk of the clip (up to 7 frames early)

__device__ __forceinline__ float s16_at(const uint4& q, int i) {          // sample i (0..7) of a 16-byte chunk of int16
    const unsigned w = i < 2 ? q.x : (i < 4 ? q.y : (i < 6 ? q.z : q.w));
    return (float)(short)(w >> ((i & 1) * 16)) * (1.f / 32768.f);
}

// frames [k0, k0 + count) of one clip -> s_x[0, count), zeros outside [0, n_in)
template <int FMT> __device__ __forceinline__ void load_span(float* s_x, const unsigned char* clip, long k0, int count, long n_in, int channels) {
    const int fb = channels * sample_bytes(FMT);
    for (int i = threadIdx.x; i < count; i += THREADS) {
        const long k = k0 + i;
        s_x[i] = (k >= 0 && k < n_in) ? decode_frame<FMT>(clip + k * fb, channels) : 0.f;
    }
}

// int16 with CH in {1, 2} from a 16-byte aligned clip: one 16-byte load per 8 / CH frames.  k0 is a multiple of 8 / CH, count too.
template <int CH> __device__ __forceinline__ void load_span_s16_vec(float* s_x, const unsigned char* clip, long k0, int count, long n_in) {
    constexpr int FPC = 8 / CH;
    for (int c = threadIdx.x; c < count / FPC; c += THREADS) {
        const long k = k0 + (long)c * FPC;
        float v[FPC];
        if (k >= 0 && k + FPC <= n_in) {
            const uint4 q = *(const uint4*)(clip + k * (2 * CH));
#pragma unroll
            for (int f = 0; f < FPC; ++f) v[f] = CH == 1 ? s16_at(q, f) : (s16_at(q, 2 * f) + s16_at(q, 2 * f + 1)) / 2.f;
        } else {
#pragma unroll
            for (int f = 0; f < FPC; ++f) v[f] = (k + f >= 0 && k + f < n_in) ? decode_frame<EMAGE_PCM_S16>(clip + (k + f) * (2 * CH), CH) : 0.f;
        }
#pragma unroll
        for (int f = 0; f < FPC; f += 4) *(float4*)(s_x + c * FPC + f) = make_float4(v[f], v[f + 1], v[f + 2], v[f + 3]);
    }
}

// VEC: 0 = any format, per-sample loads; 1 / 2 = int16 mono / stereo through 16-byte loads
template <int FMT, int VEC>
__global__ __launch_bounds__(THREADS) void audio_resample_kernel(const unsigned char* __restrict__ pcm, long pitch, int channels, long n_in,
                                                                 const float* __restrict__ taps, int table, int rpp, int row_pitch, int half, int up, int down,
                                                                 float* __restrict__ out, long ldo, long n_out, int n_tiles, int span_cap) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* s_h = smem;                                   // up rows of row_pitch taps
    float* s_x = smem + ((table + 3) & ~3);              // span_cap decoded mono samples (16-byte aligned)
    const unsigned char* clip = pcm + (long)blockIdx.y * pitch;
    float* orow = out + (long)blockIdx.y * ldo;
    for (int i = threadIdx.x; i < table / 4; i += THREADS) ((float4*)s_h)[i] = ((const float4*)taps)[i];
    for (int i = (table & ~3) + threadIdx.x; i < table; i += THREADS) s_h[i] = taps[i];
    constexpr int FPC = VEC ? 8 / VEC : 1;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const long m0 = (long)tile * TILE;
        const int rows = (int)(n_out - m0 < TILE ? n_out - m0 : TILE);
        const long base0 = m0 * down + half;             // 64-bit: m*down passes 2^31 for long clips at high rates
        const long q0 = base0 / up;
        const int r0 = (int)(base0 % up);
        long k0 = q0 - (rpp - 1);                        // first frame any output of the tile reads
        k0 -= ((k0 % FPC) + FPC) % FPC;                  // ... moved down to the start of its 16-byte chunk
        int count = (int)(q0 + ((long)(rows - 1) * down + r0) / up - k0) + 1;
        count = (count + FPC - 1) / FPC * FPC;
        if (count > span_cap) count = span_cap;          // never true for the span_cap the host computes from the same numbers
        __syncthreads();                                 // the previous tile's readers are done with s_x
        if constexpr (VEC) load_span_s16_vec<VEC>(s_x, clip, k0, count, n_in);
        else load_span<FMT>(s_x, clip, k0, count, n_in, channels);
        __syncthreads();
        const int xoff = (int)(q0 - k0);
        for (int r = threadIdx.x; r < rows; r += THREADS) {
            const int d = r * down + r0;                 // (m*down + half) - q0*up; fits 32 bits: TILE*down + up < 2^31 is checked on the host
            const float* __restrict__ h = s_h + (d % up) * row_pitch;
            const float* __restrict__ x = s_x + xoff + d / up;
            float acc = 0.f;
            for (int i = 0; i < rpp; ++i) acc = emage_pcm::tap_step(acc, h, x, i);
            orow[m0 + r] = acc;
        }
    }
}

// up == down == 1: decode and down-mix only
template <int FMT>
__global__ __launch_bounds__(THREADS) void audio_decode_kernel(const unsigned char* __restrict__ pcm, long pitch, int channels, long n_in,
                                                               float* __restrict__ out, long ldo) {
    const unsigned char* clip = pcm + (long)blockIdx.y * pitch;
    const int fb = channels * sample_bytes(FMT);
    for (long k = (long)blockIdx.x * THREADS + threadIdx.x; k < n_in; k += (long)gridDim.x * THREADS)
        out[(long)blockIdx.y * ldo + k] = decode_frame<FMT>(clip + k * fb, channels);
}

template <int FMT, int VEC, typename... A> int launch_resample(dim3 grid, size_t lds, hipStream_t s, A... args) {
    static const hipError_t configured = hipFuncSetAttribute((const void*)audio_resample_kernel<FMT, VEC>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (configured != hipSuccess) return (int)configured;
    hipLaunchKernelGGL((audio_resample_kernel<FMT, VEC>), grid, dim3(THREADS), lds, s, args...);
    return launch_status();
}

}  // namespace

extern "C" int emage_audio_resample(int fmt, const void* pcm, long clip_pitch_bytes, int channels, long n_in,
                                    const float* taps, int n_taps, int up, int down,
                                    float* out, long ldo, long n_out, int n_clips, void* stream) {
    if (!pcm || !out || fmt < EMAGE_PCM_S16 || fmt > EMAGE_PCM_F32 || channels < 1 || channels > 8) return EMAGE_EINVAL;
    if (n_in <= 0 || n_clips <= 0 || n_clips > 65535 || up <= 0 || down <= 0 || up > (1 << 16) || down > (1 << 16)) return EMAGE_EINVAL;
    if (n_out != (n_in * up + down - 1) / down || ldo < n_out) return EMAGE_EINVAL;
    const int sb = sample_bytes(fmt);
    if (clip_pitch_bytes < n_in * channels * sb) return EMAGE_EINVAL;
    if (sb != 3 && (((uintptr_t)pcm | (uintptr_t)clip_pitch_bytes) & (sb - 1))) return EMAGE_EINVAL;      // samples at their natural alignment
    hipStream_t s = (hipStream_t)stream;
    const auto* p = (const unsigned char*)pcm;
    if (up == 1 && down == 1) {
        long bx = (n_in + THREADS - 1) / THREADS;
        const dim3 grid((unsigned)(bx > 4096 ? 4096 : bx), n_clips);
#define EMAGE_DECODE(F) hipLaunchKernelGGL((audio_decode_kernel<F>), grid, dim3(THREADS), 0, s, p, clip_pitch_bytes, channels, n_in, out, ldo)
        if (fmt == EMAGE_PCM_S16) EMAGE_DECODE(EMAGE_PCM_S16);
        else if (fmt == EMAGE_PCM_S24) EMAGE_DECODE(EMAGE_PCM_S24);
        else if (fmt == EMAGE_PCM_S32) EMAGE_DECODE(EMAGE_PCM_S32);
        else EMAGE_DECODE(EMAGE_PCM_F32);
#undef EMAGE_DECODE
        return launch_status();
    }
    const int mx = up > down ? up : down, half = 10 * mx;
    if (!taps || n_taps != 2 * half + 1 || ((uintptr_t)taps & 15)) return EMAGE_EINVAL;
    const int rpp = (n_taps + up - 1) / up;              // taps of the longest phase
    const int row_pitch = rpp | 1;
    const long table = (long)up * row_pitch;
    const long span_cap = ((long)(TILE - 1) * down + up - 1) / up + rpp + 1 + SPAN_SLACK;
    if (table * 4 > EMAGE_AUDIO_TAPS_LDS_BYTES || span_cap * 4 > EMAGE_AUDIO_SPAN_LDS_BYTES) return EMAGE_EINVAL;
    const size_t lds = (size_t)(((table + 3) & ~3L) + span_cap) * sizeof(float);
    const int n_tiles = (int)((n_out + TILE - 1) / TILE);
    int cus = device_cus();
    if (cus <= 0) cus = 256;
    int gx = (3 * cus + n_clips - 1) / n_clips;          // about three blocks per CU; a block keeps its phase rows for all of its tiles
    if (gx > n_tiles) gx = n_tiles;
    const dim3 grid(gx, n_clips);
#define EMAGE_RESAMPLE(F, V) launch_resample<F, V>(grid, lds, s, p, clip_pitch_bytes, channels, n_in, taps, (int)table, rpp, row_pitch, half, up, down, out, ldo, n_out, n_tiles, (int)span_cap)
    const bool vec = fmt == EMAGE_PCM_S16 && channels <= 2 && !(((uintptr_t)pcm | (uintptr_t)clip_pitch_bytes) & 15);
    if (vec) return channels == 1 ? EMAGE_RESAMPLE(EMAGE_PCM_S16, 1) : EMAGE_RESAMPLE(EMAGE_PCM_S16, 2);
    if (fmt == EMAGE_PCM_S16) return EMAGE_RESAMPLE(EMAGE_PCM_S16, 0);
    if (fmt == EMAGE_PCM_S24) return EMAGE_RESAMPLE(EMAGE_PCM_S24, 0);
    if (fmt == EMAGE_PCM_S32) return EMAGE_RESAMPLE(EMAGE_PCM_S32, 0);
    return EMAGE_RESAMPLE(EMAGE_PCM_F32, 0);
#undef EMAGE_RESAMPLE
}
