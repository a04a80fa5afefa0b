// What the weight-streaming kernels of csrc/gemv.hip (bf16 weights) and csrc/gemv_fp8.hip (e4m3fn weights) share: the dot2 step, the
// non-temporal weight load, the LDS staging of RMS-normalised batch rows, and the host side's run-time -> compile-time row counts.
#pragma once
#include "common.h"
#include <type_traits>

typedef __bf16 dot_bf16x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ float dot8(const uint4& a, const uint4& b, float acc) {
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(dot_bf16x2, a.x), __builtin_bit_cast(dot_bf16x2, b.x), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(dot_bf16x2, a.y), __builtin_bit_cast(dot_bf16x2, b.y), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(dot_bf16x2, a.z), __builtin_bit_cast(dot_bf16x2, b.z), acc, false);
    acc = __builtin_amdgcn_fdot2_f32_bf16(__builtin_bit_cast(dot_bf16x2, a.w), __builtin_bit_cast(dot_bf16x2, b.w), acc, false);
    return acc;
}

__device__ __forceinline__ uint4 ld_stream(const uint4* p) {
    typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
    u32x4 v = __builtin_nontemporal_load((const u32x4*)p);
    return make_uint4(v[0], v[1], v[2], v[3]);
}

// STAGE: wave m of the workgroup normalises batch row m (and m + 4 when M > 4) ONCE into LDS and every wave's trips read it from there.
// Two things were wrong with every wave rebuilding the normalised slices itself: the sum of squares was a loop of one 16-byte
// load + s_waitcnt vmcnt(0) per 64-vector slice -- eight dependent L2 round trips per row, queued BEHIND the weight prefetch
// (vmcnt retires in order), ~6 us of every wave's life at M = 1 -- and at M >= 2 the per-trip re-normalisation made the
// launches VALU-bound (fused Hyena step 22 / 26 / 43 us at M = 1 / 2 / 4 against 20-22 us for the plain GEMV of the matrix).
// Here the staging wave requests its row's 2 x 8 vectors at once, AHEAD of its weight prefetch, reduces in rmsnorm_kernel's
// order (lane-strided sequential fp32, wave butterfly) and stores the normalised row: bit-identical values, one L2 round trip.
#define GV_WG_BARRIER() asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory")   // orders LDS only: weight loads stay in flight
extern __shared__ uint4 gv_xn[];                                                          // [M][nvec] normalised rows (STAGE)

__device__ __forceinline__ uint4 gv_norm8(const uint4& xv, const uint4& sv, float inv) {
    uint4 o;
    o.x = pack_bf2(bf_lo(sv.x) * (bf_lo(xv.x) * inv), bf_hi(sv.x) * (bf_hi(xv.x) * inv));
    o.y = pack_bf2(bf_lo(sv.y) * (bf_lo(xv.y) * inv), bf_hi(sv.y) * (bf_hi(xv.y) * inv));
    o.z = pack_bf2(bf_lo(sv.z) * (bf_lo(xv.z) * inv), bf_hi(sv.z) * (bf_hi(xv.z) * inv));
    o.w = pack_bf2(bf_lo(sv.w) * (bf_lo(xv.w) * inv), bf_hi(sv.w) * (bf_hi(xv.w) * inv));
    return o;
}
__device__ __forceinline__ float gv_sumsq8(const uint4& xv, float ss) {
    const float f[8] = {bf_lo(xv.x), bf_hi(xv.x), bf_lo(xv.y), bf_hi(xv.y), bf_lo(xv.z), bf_hi(xv.z), bf_lo(xv.w), bf_hi(xv.w)};
#pragma unroll
    for (int e = 0; e < 8; ++e) ss = fmaf(f[e], f[e], ss);
    return ss;
}
// rows of up to 512 vectors (the host stages K = 4096 only; other widths take the unstaged kernels): request everything (slices
// past the row end re-read the lane's first vector, unused)
__device__ __forceinline__ void gv_stage_load(const uint4* xr, const uint4* scale, int nvec, int lane, uint4 (&sx)[8], uint4 (&sc)[8]) {
    const int v0 = lane < nvec ? lane : 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int v = lane + 64 * i, vc = v < nvec ? v : v0;
        sx[i] = xr[vc];
        sc[i] = scale[vc];
    }
}
__device__ __forceinline__ void gv_stage_finish(uint4* dst, int nvec, int lane, float eps, float inv_sqrt_d, const uint4 (&sx)[8],
                                                const uint4 (&sc)[8]) {
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (lane + 64 * i < nvec) ss = gv_sumsq8(sx[i], ss);
    ss = wave_sum(ss);
    const float inv = 1.0f / (sqrtf(ss) * inv_sqrt_d + eps);
    uint4 px[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {                            // (opaque copy: otherwise the 64 unpacked fp32 values of the reduction are
        px[i] = sx[i];                                       //  kept alive across it for the normalisation, +64 VGPRs on every wave)
        asm volatile("" : "+v"(px[i].x), "+v"(px[i].y), "+v"(px[i].z), "+v"(px[i].w));
    }
#pragma unroll
    for (int i = 0; i < 8; ++i)
        if (lane + 64 * i < nvec) dst[lane + 64 * i] = gv_norm8(px[i], sc[i], inv);
}

// host side: compile-time constants from run-time row counts, as f(gv_int<V>).  for_m: the dot2 kernels' M (1 <= M <= 8: the callers
// check).  for_m_stage: the norm-folding kernels' (M, STAGE), as f(gv_int<M>, std::bool_constant<STAGE>) -- they exist LDS-staged
// (K = 4096) for 1-8 rows and unstaged for 1-4, and nothing else is instantiated.
template <int V> using gv_int = std::integral_constant<int, V>;
template <int V = 1, class F>
static void for_m(int64_t M, F f) {
    if constexpr (V == 8) f(gv_int<8>{}); else if (M == V) f(gv_int<V>{}); else for_m<V + 1>(M, f);
}
template <class F>
static void for_m_stage(int64_t M, bool stage, F f) {
    for_m(M, [&](auto m) {
        if (stage) f(m, std::true_type{}); else if constexpr (decltype(m)::value <= 4) f(m, std::false_type{});
    });
}
