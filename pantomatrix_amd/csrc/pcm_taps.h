// PCM decode, channel mean and the per-output tap walk of the polyphase resampler — shared by the whole-clip front end (audio.hip) and the
// streaming one (stream.hip: emage_stream_push_resample), so the two cannot drift: a streamed session's samples equal the offline pass over
// the same PCM bit for bit only while both sum the same products in the same order.
#pragma once
#include "common.h"

namespace emage_pcm {

constexpr int SPAN_SLACK = 16;                // floats a tile's LDS span holds beyond its frames: part of the span budget both kernels accept rates by

__host__ __device__ constexpr int sample_bytes(int fmt) { return fmt == EMAGE_PCM_S16 ? 2 : (fmt == EMAGE_PCM_S24 ? 3 : 4); }

template <int FMT> __device__ __forceinline__ float decode_sample(const unsigned char* p) {
    if constexpr (FMT == EMAGE_PCM_S16) return (float)*(const short*)p * (1.f / 32768.f);
    else if constexpr (FMT == EMAGE_PCM_S24) {
        const int v = (int)p[0] | ((int)p[1] << 8) | ((int)p[2] << 16);
        return (float)((v ^ 0x800000) - 0x800000) * (1.f / 8388608.f);
    } else if constexpr (FMT == EMAGE_PCM_S32) return (float)*(const int*)p * (1.f / 2147483648.f);      // int -> float rounds to nearest even
    else return *(const float*)p;
}

// one frame -> mono: the fp32 sum in channel order over the channel count (one channel: no arithmetic)
template <int FMT> __device__ __forceinline__ float decode_frame(const unsigned char* p, int channels) {
    float s = decode_sample<FMT>(p);
    if (channels == 1) return s;
    for (int c = 1; c < channels; ++c) s += decode_sample<FMT>(p + c * sample_bytes(FMT));
    return s / (float)channels;
}

// tap i of one output: phase row h[0 .. rpp) against x[0], x[-1], ... x[-(rpp - 1)].  An output is this step from acc = 0 over i = 0 .. rpp - 1,
// in that order; the loop stands in each kernel (hoisted into a function here, the whole-clip kernels compile to other code than before)
__device__ __forceinline__ float tap_step(float acc, const float* h, const float* x, int i) { return fmaf(h[i], x[-i], acc); }

}  // namespace emage_pcm
