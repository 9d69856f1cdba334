// One step of the root-translation scan (`velocity2position`, P:107-115): pos[t] = v[t-1] * dt + pos[t-1], the product and the sum each
// rounded to fp32 — the reference's rounding order is part of the contract.  Shared by the whole-sequence scan (motion.hip) and the scan
// that continues across the segments of a stream (stream.hip), so the two cannot drift.
#pragma once
#include <hip/hip_runtime.h>

namespace emage_vel {

__device__ __forceinline__ float step(float pos, float v, float dt) { return __fadd_rn(__fmul_rn(v, dt), pos); }

}  // namespace emage_vel
