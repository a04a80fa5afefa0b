// The FP8 (OCP e4m3fn) quantisation rule, device side, shared by the KV cache (csrc/kv_fp8.hip) and the decode weights (csrc/gemv_fp8.hip).
//
// A row of bf16 values with a = max |x_j| is stored as bytes RNE_e4m3fn(x_j 2^-e) and ONE f32 scale 2^e, where e is the smallest integer
// with a 2^-e <= 448, clamped to [-126, 120] (a = 0: e = 0).  x_j 2^-e is exact in fp32 and at most 448 in magnitude, so the conversion
// rounds once and never saturates; byte * scale is exact in fp32.  e comes from the exponent and mantissa bits of a (a bf16 value:
// 448 = 1.75 * 2^8, so the mantissa decides between two neighbouring exponents), never from a logarithm.
#pragma once
#include "common.h"

// e of the rule from max |x| given as the 15 magnitude bits of a bf16 (exponent field E, 7 mantissa bits M): a = 1.M 2^(E-127), and
// 1.M <= 1.75 <=> M <= 0x60.  A subnormal a (E = 0) lands below the clamp.
__device__ __forceinline__ int fp8_row_exponent(uint32_t amax15) {
    if (amax15 == 0) return 0;
    const int e = (int)(amax15 >> 7) - 135 + ((amax15 & 0x7f) > 0x60 ? 1 : 0);
    return e < -126 ? -126 : e;
}
__device__ __forceinline__ float fp8_pow2(int e) { return __uint_as_float((uint32_t)(127 + e) << 23); }    // e in [-126, 126]

__device__ __forceinline__ uint32_t fp8_max15(const uint4& v) {
    uint32_t m = max(v.x & 0x7fffu, (v.x >> 16) & 0x7fffu);
    m = max(m, max(v.y & 0x7fffu, (v.y >> 16) & 0x7fffu));
    m = max(m, max(v.z & 0x7fffu, (v.z >> 16) & 0x7fffu));
    return max(m, max(v.w & 0x7fffu, (v.w >> 16) & 0x7fffu));
}
template <int CTRL>
__device__ __forceinline__ uint32_t fp8_dpp_u32(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xf, 0xf, true);
}
// maximum over the 8 (16) lanes of an aligned lane group, DPP only (see wave_max in common.h for why the mirrors stand in for xor 4 / 8)
template <int LANES>
__device__ __forceinline__ uint32_t fp8_group_max(uint32_t v) {
    v = max(v, fp8_dpp_u32<EVO_DPP_XOR1>(v));
    v = max(v, fp8_dpp_u32<EVO_DPP_XOR2>(v));
    v = max(v, fp8_dpp_u32<EVO_DPP_HALF_MIRROR>(v));
    if (LANES == 16) v = max(v, fp8_dpp_u32<EVO_DPP_MIRROR>(v));
    return v;
}
// 8 bf16 values times the (exact) factor `inv` -> 8 e4m3fn bytes in memory order (v_cvt_pk_fp8_f32: round to nearest even)
__device__ __forceinline__ uint2 fp8_quant8(const uint4& v, float inv) {
    int lo = 0, hi = 0;
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(bf_lo(v.x) * inv, bf_hi(v.x) * inv, lo, false);
    lo = __builtin_amdgcn_cvt_pk_fp8_f32(bf_lo(v.y) * inv, bf_hi(v.y) * inv, lo, true);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(bf_lo(v.z) * inv, bf_hi(v.z) * inv, hi, false);
    hi = __builtin_amdgcn_cvt_pk_fp8_f32(bf_lo(v.w) * inv, bf_hi(v.w) * inv, hi, true);
    return make_uint2((uint32_t)lo, (uint32_t)hi);
}
