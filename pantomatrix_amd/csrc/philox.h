// Philox4x32-10 (Salmon et al., SC'11), the counter-based generator behind every mask this library draws on the device: emage_dropout_mask /
// emage_mul_add_philox (train.hip) and emage_motion_mask (data.hip).  One convention for all of them:
//   key = (seed lo, seed hi);  counter = (i / 4 lo, i / 4 hi, mask id, step);  element i takes word i % 4 of the block;
//   u_i = (word >> 8) * 2^-24      (24 random bits, uniform on [0, 1), exact in fp32)
// The stream is this library's own, pinned bit for bit by tests/test_train_rng.py against a numpy Philox; it is NOT torch's.
#pragma once
#include <hip/hip_runtime.h>

__device__ __forceinline__ void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned long long p0 = (unsigned long long)0xD2511F53u * c[0], p1 = (unsigned long long)0xCD9E8D57u * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n1 = (unsigned)p1, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1, n3 = (unsigned)p0;
        c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

__device__ __forceinline__ float philox_uniform(unsigned word) { return (float)(word >> 8) * (1.0f / 16777216.0f); }
