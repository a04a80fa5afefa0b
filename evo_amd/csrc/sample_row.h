// What the kernels over one [512] row of logits share (csrc/sample.hip: the seeded draw; csrc/beam.hip: the beam selection): the
// order-preserving 32-bit pattern of a float, the integer wave sum, the row load and the log-sum-exp of the unfiltered row in its FIXED
// order.  One 64-lane wave per row; lane l holds ids 8 l ... 8 l + 7.
#pragma once
#include "common.h"

#define EVO_SAMPLE_V 512

// float <-> a 32-bit pattern whose unsigned order is the float order (-inf lowest, +inf highest)
__device__ __forceinline__ uint32_t sample_ord(float x) {
    const uint32_t u = __float_as_uint(x);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sample_unord(uint32_t o) {
    return __uint_as_float((o & 0x80000000u) ? (o ^ 0x80000000u) : ~o);
}

__device__ __forceinline__ int sample_wave_sum_i(int v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// log-sum-exp of the UNFILTERED row (fp32), in its FIXED order: 8 sequential terms per lane, then the butterfly over the lanes.  A macro,
// not a function: declares `lse` (and the temporaries lse_mx / lse_se) in the caller's scope
#define EVO_SAMPLE_ROW_LSE(x, lse)                                  \
    float lse_mx = (x)[0];                                          \
    _Pragma("unroll")                                               \
    for (int j = 1; j < 8; ++j) lse_mx = fmaxf(lse_mx, (x)[j]);     \
    lse_mx = wave_max(lse_mx);                                      \
    float lse_se = 0.f;                                             \
    _Pragma("unroll")                                               \
    for (int j = 0; j < 8; ++j) lse_se += expf((x)[j] - lse_mx);    \
    lse_se = wave_sum(lse_se);                                      \
    const float lse = lse_mx + logf(lse_se);
