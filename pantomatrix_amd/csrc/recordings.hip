// Data movement of the lock-step pass over recordings of different lengths (pantomatrix_amd/recordings.py: the reference's test pass,
// train_emage_audio.py:33-102, as a static schedule of ordinary batches).  Two table-driven copies, so that the pass reads no host state:
//   emage_gather_windows  ONE launch fills a contiguous (n, samples) fp32 batch of audio windows out of the flat array that holds every
//                         recording end to end (s16 decoded x * 2^-15, or float32 — the convention of emage_gather_clips); row b starts at
//                         sample offsets[b], so the rows of one batch come from different recordings at different frames.
//   emage_copy_segments   ONE launch copies segments {first source row, first destination row, rows} of `width`-byte rows between two
//                         buffers: a tail group's codes into each recording's slot, seed rows / ref_trans of a group, the results of every
//                         recording into one flat buffer per output.
// A block serves one row / one span of one segment; no LDS.  A window starts at any sample (a frame is 533 samples) and a segment at any row,
// so a 16-byte access is aligned only from some element on: a row is a scalar head up to the first 16-byte boundary of the SOURCE, 16-byte
// loads from there (stored with 16-byte stores when the destination happens to be aligned at the same element, else element by element), and
// a scalar tail.  A row / segment that does not lie inside its arrays is reported in the status word and reads nothing: the window is
// zero-filled, the segment is skipped.
#include "common.h"

namespace {

constexpr int THREADS = 256;
constexpr long SEG_SPAN = 64 * 1024;          // bytes of a segment one block copies (256 per thread)

template <int FMT> struct Pcm;
template <> struct Pcm<EMAGE_PCM_S16> {
    typedef short T;
    __device__ static __forceinline__ float decode(short v) { return (float)v * (1.f / 32768.f); }
    __device__ static __forceinline__ void unpack(const uint4& r, float* v) {
        const unsigned w[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            v[2 * k] = decode((short)(w[k] & 0xffffu));
            v[2 * k + 1] = decode((short)(w[k] >> 16));
        }
    }
};
template <> struct Pcm<EMAGE_PCM_F32> {
    typedef float T;
    __device__ static __forceinline__ float decode(float v) { return v; }
    __device__ static __forceinline__ void unpack(const uint4& r, float* v) {
        v[0] = __builtin_bit_cast(float, r.x); v[1] = __builtin_bit_cast(float, r.y);
        v[2] = __builtin_bit_cast(float, r.z); v[3] = __builtin_bit_cast(float, r.w);
    }
};

template <int FMT>
__global__ __launch_bounds__(THREADS) void gather_windows_kernel(const void* __restrict__ audio, long total_samples, const long long* __restrict__ offsets,
                                                                 int samples, float* __restrict__ out, long ld, int* __restrict__ status) {
    typedef typename Pcm<FMT>::T T;
    constexpr int G = 16 / (int)sizeof(T);                           // samples per 16-byte load
    const int tid = threadIdx.x;
    float* o = out + (long)blockIdx.x * ld;
    const long s0 = offsets[blockIdx.x];
    if (s0 < 0 || s0 > total_samples - samples) {
        if (tid == 0) atomicOr(status, 1);
        for (int i = tid; i < samples; i += THREADS) o[i] = 0.f;
        return;
    }
    const T* src = (const T*)audio + s0;
    int head = (int)(((16 - ((uintptr_t)src & 15)) & 15) / sizeof(T));
    if (head > samples) head = samples;
    const int groups = (samples - head) / G;
    const int tail0 = head + groups * G;
    for (int i = tid; i < head; i += THREADS) o[i] = Pcm<FMT>::decode(src[i]);
    for (int i = tail0 + tid; i < samples; i += THREADS) o[i] = Pcm<FMT>::decode(src[i]);
    const bool dst16 = ((uintptr_t)(o + head) & 15) == 0;            // one answer per row: the groups are G floats apart
    for (int g = tid; g < groups; g += THREADS) {
        const int i = head + g * G;
        float v[G];
        Pcm<FMT>::unpack(*(const uint4*)(src + i), v);
        if (dst16) {
#pragma unroll
            for (int k = 0; k < G; k += 4) *(float4*)(o + i + k) = make_float4(v[k], v[k + 1], v[k + 2], v[k + 3]);
        } else {
#pragma unroll
            for (int k = 0; k < G; ++k) o[i + k] = v[k];
        }
    }
}

__global__ __launch_bounds__(THREADS) void copy_segments_kernel(const char* __restrict__ src, long src_rows, char* __restrict__ dst, long dst_rows,
                                                                const long long* __restrict__ segments, long width, long max_rows,
                                                                int* __restrict__ status) {
    const int tid = threadIdx.x;
    const long long* seg = segments + (long)blockIdx.x * 3;
    const long sr = seg[0], dr = seg[1], rows = seg[2];
    if (rows < 0 || rows > max_rows || sr < 0 || sr > src_rows - rows || dr < 0 || dr > dst_rows - rows) {
        if (tid == 0 && blockIdx.y == 0) atomicOr(status, 2);
        return;
    }
    const long bytes = rows * width;
    const long lo = (long)blockIdx.y * SEG_SPAN;
    if (lo >= bytes) return;
    const long n = bytes - lo < SEG_SPAN ? bytes - lo : SEG_SPAN;
    const char* s = src + sr * width + lo;
    char* d = dst + dr * width + lo;
    if ((((uintptr_t)s ^ (uintptr_t)d) & 15) == 0) {                 // source and destination reach a 16-byte boundary at the same byte
        long head = (long)((16 - ((uintptr_t)s & 15)) & 15);
        if (head > n) head = n;
        const long groups = (n - head) >> 4;
        const long tail0 = head + (groups << 4);
        for (long i = tid; i < head; i += THREADS) d[i] = s[i];
        for (long i = tail0 + tid; i < n; i += THREADS) d[i] = s[i];
        for (long g = tid; g < groups; g += THREADS) *(uint4*)(d + head + (g << 4)) = *(const uint4*)(s + head + (g << 4));
    } else if ((((uintptr_t)s | (uintptr_t)d | (uintptr_t)n) & 3) == 0) {
        for (long i = tid; i < (n >> 2); i += THREADS) ((unsigned*)d)[i] = ((const unsigned*)s)[i];
    } else {
        for (long i = tid; i < n; i += THREADS) d[i] = s[i];
    }
}

}  // namespace

extern "C" int emage_gather_windows(int audio_fmt, const void* audio, long total_samples, const long long* offsets, int n, int samples,
                                    float* out, long ld_out, int* status, void* stream) {
    if (!audio || !offsets || !out || !status) return EMAGE_EINVAL;
    if (audio_fmt != EMAGE_PCM_S16 && audio_fmt != EMAGE_PCM_F32) return EMAGE_EINVAL;
    if (n <= 0 || samples <= 0 || total_samples <= 0 || ld_out < samples) return EMAGE_EINVAL;
    if (((uintptr_t)audio & (audio_fmt == EMAGE_PCM_S16 ? 1 : 3)) || ((uintptr_t)offsets & 7) || ((uintptr_t)out & 3) || ((uintptr_t)status & 3)) return EMAGE_EINVAL;
    if (audio_fmt == EMAGE_PCM_S16)
        hipLaunchKernelGGL((gather_windows_kernel<EMAGE_PCM_S16>), dim3((unsigned)n), dim3(THREADS), 0, (hipStream_t)stream, audio, total_samples, offsets,
                           samples, out, ld_out, status);
    else
        hipLaunchKernelGGL((gather_windows_kernel<EMAGE_PCM_F32>), dim3((unsigned)n), dim3(THREADS), 0, (hipStream_t)stream, audio, total_samples, offsets,
                           samples, out, ld_out, status);
    return launch_status();
}

extern "C" int emage_copy_segments(const void* src, long src_rows, void* dst, long dst_rows, const long long* segments, int n_segments,
                                   long width_bytes, long max_rows, int* status, void* stream) {
    if (!src || !dst || !segments || !status) return EMAGE_EINVAL;
    if (n_segments <= 0 || width_bytes <= 0 || max_rows <= 0 || src_rows <= 0 || dst_rows <= 0) return EMAGE_EINVAL;
    if (((uintptr_t)segments & 7) || ((uintptr_t)status & 3)) return EMAGE_EINVAL;
    if (max_rows > 0x7fffffffffffL / width_bytes) return EMAGE_EINVAL;
    const long spans = (max_rows * width_bytes + SEG_SPAN - 1) / SEG_SPAN;
    if (spans > 65535) return EMAGE_EINVAL;
    hipLaunchKernelGGL(copy_segments_kernel, dim3((unsigned)n_segments, (unsigned)spans), dim3(THREADS), 0, (hipStream_t)stream, (const char*)src, src_rows,
                       (char*)dst, dst_rows, segments, width_bytes, max_rows, status);
    return launch_status();
}
