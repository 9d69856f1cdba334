// rep15d, the motion representation the reference's BC / L1div metrics read (emage_utils/motion_rep_transfer.py:51-64), from axis-angle
// poses and the 55 SMPL-X joint positions that belong to them: per (sequence, frame, joint) 15 numbers = position, velocity (one-sided
// differences at the two ends, central ones inside), rot-6D of the pose and the angular velocity by the same differences.  One launch, one
// thread per (sequence, frame, joint), fp32 in the reference's operation order (compiled with -ffp-contract=off), plain vector stores.
#include "common.h"
#include <math.h>
#include "rot_math.h"

namespace {

constexpr int NJ = EMAGE_REP_JOINTS;             // 55: the pose layout is (T, 165)
constexpr int POSE = 3 * NJ;

__global__ void motion_rep_kernel(const float* __restrict__ poses, const float* __restrict__ joints, long ld_joints, float dt, float dt2,
                                  float* __restrict__ rep, int B, int T) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)B * T * NJ) return;
    const long row = i / NJ;                         // b * T + n
    const int j = (int)(i - row * NJ);
    const int n = (int)(row % T);
    const long lo = n == 0 ? row : row - 1, hi = n == T - 1 ? row : row + 1;      // never leaves the sequence: T >= 2
    const float div = (n == 0 || n == T - 1) ? dt : dt2;
    float* o = rep + i * 15;
    float aa[3], d6[6];
    for (int c = 0; c < 3; ++c) {
        o[c] = joints[row * ld_joints + j * 3 + c];
        o[3 + c] = (joints[hi * ld_joints + j * 3 + c] - joints[lo * ld_joints + j * 3 + c]) / div;
        aa[c] = poses[row * POSE + j * 3 + c];
        o[12 + c] = (poses[hi * POSE + j * 3 + c] - poses[lo * POSE + j * 3 + c]) / div;
    }
    emage_rot::aa_to_rot6d(aa, d6);                  // the bits of emage_axis_angle_to_rot6d
    for (int c = 0; c < 6; ++c) o[6 + c] = d6[c];
}

}  // namespace

extern "C" int emage_motion_rep(const float* poses, const float* joints, long ld_joints, float dt, float* rep, int B, int T, void* stream) {
    if (!poses || !joints || !rep || B <= 0 || T < 2 || ld_joints < POSE || !(dt > 0.f)) return EMAGE_EINVAL;
    if ((long)B * T > 0x7fffffffL * 256 / NJ) return EMAGE_EINVAL;          // the grid limit (and no overflow of the products below)
    const long total = (long)B * T * NJ;
    hipLaunchKernelGGL(motion_rep_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, poses, joints, ld_joints, dt,
                       2.f * dt, rep, B, T);
    return launch_status();
}
