// Feeding the training step from a device-resident clip store (the reference's datasets/beat2.py BEAT2DatasetEamgeFootContact.__getitem__ +
// DataLoader collation, and the random motion mask of train_emage_audio.py:163-165), with no host work per step:
//   emage_gather_clips   ONE launch cuts a batch out of the flat recording arrays: for batch row b, clip id = order[(cursor % n_batches) * batch + b],
//                        clip table row {first frame, first sample, recording id}; T frames of poses (165) / expressions (100) / trans (3) /
//                        foot contact (4) and T * samples_per_frame audio samples (s16 decoded x * 2^-15, or float32) are copied into the batch
//                        tensors.  The cursor is read from device memory, so a captured graph walks the epoch by itself.
//   emage_gather_clip_speakers   the speaker-table row of each of those clips (speakers[recording id]), for stores of more than one speaker
//   emage_motion_mask    out[i] = (u_i < a * iteration + b) ? 1 : 0 with u_i from Philox4x32-10 (philox.h), iteration read from device memory
// A block of emage_gather_clips serves a (clip, span) pair: span s of a clip is elements [s * SPAN, +SPAN) of the clip's five pieces laid end
// to end (audio, poses, expressions, trans, contact).  Every access is ONE element at its natural alignment (2 bytes for s16, 4 otherwise): a clip
// starts at any frame / any sample, rows are 165 / 100 / 3 / 4 floats wide, and the outputs may be strided views, so nothing wider is ever aligned
// by construction; lanes read and write consecutive elements, which the memory system coalesces.  A clip id outside [0, n_clips) — or a table row
// that points outside the flat arrays — zero-fills that batch row and is reported in the status word; nothing outside the arrays is read.
#include "common.h"
#include "philox.h"

namespace {

constexpr int THREADS = 256;
constexpr int SPAN = 4096;                    // elements of a clip one block copies (16 per thread)
constexpr int W_POSE = EMAGE_CLIP_POSE_DIMS, W_EXPR = EMAGE_CLIP_EXPR_DIMS, W_TRANS = EMAGE_CLIP_TRANS_DIMS, W_CONTACT = EMAGE_CLIP_CONTACT_DIMS;

struct ClipOut { float* p; long clip_pitch; long row_pitch; };       // element (b, t, c) at p[b * clip_pitch + t * row_pitch + c]

// piece element j (row j / W, column j % W) of batch row b: src is the clip's first row in the flat (frames, W) array, or NULL = zero
template <int W> __device__ __forceinline__ void copy_piece(const ClipOut& o, int b, long j, const float* __restrict__ src) {
    const long t = j / W;
    const int c = (int)(j - t * W);
    o.p[b * o.clip_pitch + t * o.row_pitch + c] = src ? src[j] : 0.f;
}

template <int FMT>
__global__ __launch_bounds__(THREADS) void gather_clips_kernel(const int* __restrict__ order, const int* __restrict__ cursor, int n_batches, int batch,
                                                               const long long* __restrict__ clips, long n_clips, int frames, int spf,
                                                               const float* __restrict__ poses, const float* __restrict__ expr, const float* __restrict__ trans,
                                                               const float* __restrict__ contact, long total_frames,
                                                               const void* __restrict__ audio, long total_samples,
                                                               float* __restrict__ out_audio, long ld_audio, ClipOut o_pose, ClipOut o_expr, ClipOut o_trans,
                                                               ClipOut o_contact, int* __restrict__ status) {
    const int b = blockIdx.y;
    int pos = *cursor % n_batches;
    if (pos < 0) pos += n_batches;                                   // a cursor set below zero still lands inside the order buffer
    const long id = order[(long)pos * batch + b];
    const long n_audio = (long)frames * spf;
    long f0 = 0, s0 = 0;
    int bad = 0;
    if (id < 0 || id >= n_clips) bad = 1;
    else {
        f0 = clips[id * 3];
        s0 = clips[id * 3 + 1];
        if (f0 < 0 || f0 > total_frames - frames || s0 < 0 || s0 > total_samples - n_audio) bad = 2;
    }
    if (bad && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(status, bad);
    const long e_pose = n_audio + (long)frames * W_POSE, e_expr = e_pose + (long)frames * W_EXPR, e_trans = e_expr + (long)frames * W_TRANS,
               e_all = e_trans + (long)frames * W_CONTACT;
    const long lo = (long)blockIdx.x * SPAN;
    const long hi = lo + SPAN < e_all ? lo + SPAN : e_all;
    for (long i = lo + threadIdx.x; i < hi; i += THREADS) {
        if (i < n_audio) {
            float v = 0.f;
            if (!bad) {
                if constexpr (FMT == EMAGE_PCM_S16) v = (float)((const short*)audio)[s0 + i] * (1.f / 32768.f);
                else v = ((const float*)audio)[s0 + i];
            }
            out_audio[b * ld_audio + i] = v;
        } else if (i < e_pose) copy_piece<W_POSE>(o_pose, b, i - n_audio, bad ? nullptr : poses + f0 * W_POSE);
        else if (i < e_expr) copy_piece<W_EXPR>(o_expr, b, i - e_pose, bad ? nullptr : expr + f0 * W_EXPR);
        else if (i < e_trans) copy_piece<W_TRANS>(o_trans, b, i - e_expr, bad ? nullptr : trans + f0 * W_TRANS);
        else copy_piece<W_CONTACT>(o_contact, b, i - e_trans, bad ? nullptr : contact + f0 * W_CONTACT);
    }
}

__global__ __launch_bounds__(THREADS) void motion_mask_kernel(float* __restrict__ out, long n, double a, double b, unsigned seed_lo, unsigned seed_hi,
                                                              unsigned mask_id, const int* __restrict__ iteration) {
    const int it = *iteration;
    const float r = (float)(a * (double)it + b);                     // the reference's Python-float ratio, rounded once for the fp32 compare
    const long nblk = (n + 3) >> 2;
    for (long q = (long)blockIdx.x * blockDim.x + threadIdx.x; q < nblk; q += (long)gridDim.x * blockDim.x) {
        unsigned c[4] = {(unsigned)q, (unsigned)(q >> 32), mask_id, (unsigned)it};
        philox4x32_10(c, seed_lo, seed_hi);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long i = 4 * q + e;
            if (i < n) out[i] = philox_uniform(c[e]) < r ? 1.f : 0.f;
        }
    }
}

// out[b] = speakers[recording of the clip batch row b takes]: the same cursor arithmetic as gather_clips_kernel, one thread per batch row
__global__ __launch_bounds__(THREADS) void gather_clip_speakers_kernel(const int* __restrict__ order, const int* __restrict__ cursor, int n_batches, int batch,
                                                                       const long long* __restrict__ clips, long n_clips,
                                                                       const int64_t* __restrict__ speakers, long n_recordings,
                                                                       int64_t* __restrict__ out, int* __restrict__ status) {
    const int b = blockIdx.x * THREADS + threadIdx.x;
    if (b >= batch) return;
    int pos = *cursor % n_batches;
    if (pos < 0) pos += n_batches;
    const long id = order[(long)pos * batch + b];
    int64_t row = 0;
    int bad = 0;
    if (id < 0 || id >= n_clips) bad = 1;
    else {
        const long r = clips[id * 3 + 2];
        if (r < 0 || r >= n_recordings) bad = 2;
        else {
            row = speakers[r];
            if (row < 0) { row = 0; bad = 2; }
        }
    }
    if (bad) atomicOr(status, bad);
    out[b] = row;
}

bool fits(long clip_pitch, long row_pitch, int frames, int width) { return row_pitch >= width && clip_pitch >= (long)(frames - 1) * row_pitch + width; }

}  // namespace

extern "C" int emage_gather_clips(const int* order, long n_order, const int* cursor, int n_batches, int batch,
                                  const long long* clips, long n_clips, int frames, int samples_per_frame,
                                  const float* poses, const float* expressions, const float* trans, const float* contact, long total_frames,
                                  int audio_fmt, const void* audio, long total_samples,
                                  float* out_audio, long ld_audio,
                                  float* out_poses, long poses_clip_pitch, long poses_row_pitch,
                                  float* out_expressions, long expressions_clip_pitch, long expressions_row_pitch,
                                  float* out_trans, long trans_clip_pitch, long trans_row_pitch,
                                  float* out_contact, long contact_clip_pitch, long contact_row_pitch,
                                  int* status, void* stream) {
    if (!order || !cursor || !clips || !poses || !expressions || !trans || !contact || !audio || !status) return EMAGE_EINVAL;
    if (!out_audio || !out_poses || !out_expressions || !out_trans || !out_contact) return EMAGE_EINVAL;
    if (audio_fmt != EMAGE_PCM_S16 && audio_fmt != EMAGE_PCM_F32) return EMAGE_EINVAL;
    if (batch <= 0 || batch > 65535 || n_batches <= 0 || frames <= 0 || samples_per_frame <= 0 || n_clips <= 0) return EMAGE_EINVAL;
    if (n_order < (long)n_batches * batch || total_frames < frames || total_samples < (long)frames * samples_per_frame) return EMAGE_EINVAL;
    if (ld_audio < (long)frames * samples_per_frame) return EMAGE_EINVAL;
    if (!fits(poses_clip_pitch, poses_row_pitch, frames, W_POSE) || !fits(expressions_clip_pitch, expressions_row_pitch, frames, W_EXPR) ||
        !fits(trans_clip_pitch, trans_row_pitch, frames, W_TRANS) || !fits(contact_clip_pitch, contact_row_pitch, frames, W_CONTACT)) return EMAGE_EINVAL;
    if (((uintptr_t)audio & (audio_fmt == EMAGE_PCM_S16 ? 1 : 3)) || ((uintptr_t)clips & 7)) return EMAGE_EINVAL;      // elements at their natural alignment
    const long per_clip = (long)frames * (samples_per_frame + W_POSE + W_EXPR + W_TRANS + W_CONTACT);
    const long spans = (per_clip + SPAN - 1) / SPAN;
    if (spans > 0x7fffffffL) return EMAGE_EINVAL;
    const dim3 grid((unsigned)spans, batch);
    const ClipOut op{out_poses, poses_clip_pitch, poses_row_pitch}, oe{out_expressions, expressions_clip_pitch, expressions_row_pitch},
                  ot{out_trans, trans_clip_pitch, trans_row_pitch}, oc{out_contact, contact_clip_pitch, contact_row_pitch};
#define EMAGE_GATHER(F) hipLaunchKernelGGL((gather_clips_kernel<F>), grid, dim3(THREADS), 0, (hipStream_t)stream, order, cursor, n_batches, batch, clips, n_clips, \
                                           frames, samples_per_frame, poses, expressions, trans, contact, total_frames, audio, total_samples, out_audio, ld_audio, \
                                           op, oe, ot, oc, status)
    if (audio_fmt == EMAGE_PCM_S16) EMAGE_GATHER(EMAGE_PCM_S16);
    else EMAGE_GATHER(EMAGE_PCM_F32);
#undef EMAGE_GATHER
    return launch_status();
}

extern "C" int emage_gather_clip_speakers(const int* order, long n_order, const int* cursor, int n_batches, int batch,
                                          const long long* clips, long n_clips, const int64_t* speakers, long n_recordings,
                                          int64_t* out, int* status, void* stream) {
    if (!order || !cursor || !clips || !speakers || !out || !status) return EMAGE_EINVAL;
    if (batch <= 0 || batch > 65535 || n_batches <= 0 || n_clips <= 0 || n_recordings <= 0 || n_order < (long)n_batches * batch) return EMAGE_EINVAL;
    if (((uintptr_t)clips & 7) || ((uintptr_t)speakers & 7) || ((uintptr_t)out & 7)) return EMAGE_EINVAL;
    hipLaunchKernelGGL(gather_clip_speakers_kernel, dim3((unsigned)((batch + THREADS - 1) / THREADS)), dim3(THREADS), 0, (hipStream_t)stream, order, cursor,
                       n_batches, batch, clips, n_clips, speakers, n_recordings, out, status);
    return launch_status();
}

extern "C" int emage_motion_mask(float* out, long n, double a, double b, unsigned long long seed, unsigned mask_id, const int* iteration, void* stream) {
    if (!out || !iteration || n <= 0 || !(a == a) || !(b == b)) return EMAGE_EINVAL;
    long blocks = ((n + 3) / 4 + THREADS - 1) / THREADS;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(motion_mask_kernel, dim3((unsigned)blocks), dim3(THREADS), 0, (hipStream_t)stream, out, n, a, b,
                       (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), mask_id, iteration);
    return launch_status();
}
