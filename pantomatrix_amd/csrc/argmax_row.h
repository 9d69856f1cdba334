// The classifier row of vq.hip (emage_argmax_logsoftmax_f32) and val.hip (emage_val_metrics): one wave's fp32 log-softmax of a row and the
// first maximum of it.  ONE statement of the arithmetic — lane l takes columns l, l + 64, ... in rising order, the wave folds by xor
// butterflies — so both kernels return the same index for the same logits, ties and NaN rows included.
#pragma once
#include "common.h"
#include <math.h>

// (value, index) "greater" with torch's rules: the first extremum wins ties, and a NaN is the extremum (torch.argmax / max return the
// position of the first NaN), so a NaN upstream surfaces as its own index instead of a plausible-looking code
__device__ __forceinline__ void take_max(float& d, int& i, float od, int oi) {
    const bool od_nan = od != od, d_nan = d != d;
    if (od > d || (od == d && oi < i) || (od_nan && (!d_nan || oi < i))) { d = od; i = oi; }
}

// Index tensors are addressed as 2-D views: element n of a flat (N,) index list lives at (n / rows)*ld + (n % rows)*ts,
// so a (B, T) window cut out of a longer (B, L) code buffer (ld = L), or one id per clip broadcast over T frames
// (ts = 0), is read / written in place.  rows <= 0 means a plain contiguous list.
struct IdxView { int rows; long ld; int ts; };
__device__ __forceinline__ long idx_at(const IdxView v, int n) {
    if (v.rows <= 0) return n;
    const int b = n / v.rows;
    return (long)b * v.ld + (long)(n - b * v.rows) * v.ts;
}

// y[c] = (x[c] - max) - log(sum exp(x - max)) over the C columns `at(c)` of one row, by the 64 lanes of a wave: every lane returns the row
// maximum mx, ls = log(sum) and the first maximum of y (value bd, column bi).
template <typename At>
__device__ __forceinline__ void row_logsoftmax_argmax(At at, int C, int lane, float& mx, float& ls, float& bd, int& bi) {
    mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, at(c));
    for (int m = 32; m >= 1; m >>= 1) mx = fmaxf(mx, __shfl_xor(mx, m));
    float sum = 0.f;
    for (int c = lane; c < C; c += 64) sum += expf(at(c) - mx);
    for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m);
    ls = logf(sum);
    bd = -INFINITY; bi = 0x7fffffff;
    for (int c = lane; c < C; c += 64) take_max(bd, bi, __fsub_rn(__fsub_rn(at(c), mx), ls), c);
    for (int m = 32; m >= 1; m >>= 1) {
        const float od = __shfl_xor(bd, m); const int oi = __shfl_xor(bi, m);
        take_max(bd, bi, od, oi);
    }
}
