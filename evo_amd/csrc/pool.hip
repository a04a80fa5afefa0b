// Masked row pooling of the residual stream (sequence embeddings), with the final RMSNorm optionally fused in.
// HBM-bound: every pooled row is read once, 16 bytes per lane; nothing of size [rows, D] is written.  Two launches:
//   (1) pool_strip_kernel: a workgroup owns one strip of rows of one sequence; each of its 4 waves takes every 4th row of the
//       strip (one wave per row: the sum of squares is a wave reduction), keeps the D / 64 fp32 column sums of its rows in
//       registers, the 4 waves meet in LDS in a fixed order and the workgroup stores its fp32 partial slab [D];
//   (2) pool_finish_kernel: the slabs of every sequence are added in a fixed order, scaled by 1 / n and, with the norm, by `scale`.
// No float atomics anywhere: the result is bit-identical from run to run.  Entry point and contract: include/evo_mi355x.h.
#include "common.h"
#include "../../include/evo_mi355x.h"

#define EVO_POOL_MAX_D 4096          // register plan: D / 512 16-byte vectors per lane, at most 8

__device__ __forceinline__ void pool_unpack8(const uint4& v, float* f) {
    f[0] = bf_lo(v.x); f[1] = bf_hi(v.x); f[2] = bf_lo(v.y); f[3] = bf_hi(v.y);
    f[4] = bf_lo(v.z); f[5] = bf_hi(v.z); f[6] = bf_lo(v.w); f[7] = bf_hi(v.w);
}

// The rows a strip pools: mode 0 (mean) splits [first, first + n) into n_strips nearly equal pieces, mode 1 (last) gives the last
// row to strip 0.  A range outside [0, M) pools nothing here; pool_finish_kernel writes NaN for it.  (No first + n: a device-side
// pair such as (2^62, 2^62) wraps that sum in int64 and would pass.)
__device__ __forceinline__ bool pool_range_ok(int64_t first, int64_t n, int64_t M) {
    return first >= 0 && n >= 1 && first <= M && n <= M - first;
}

template <int NV, bool NORM>   // NV = 16-byte vectors per lane (D <= NV * 512)
__global__ __launch_bounds__(256) void pool_strip_kernel(const uint4* __restrict__ x, int64_t M, int nvec, int64_t ld_vec,
                                                         const int64_t* __restrict__ ranges, int mode, int n_strips, float eps,
                                                         float inv_sqrt_d, float* __restrict__ ws) {
    __shared__ float red[2][NV * 512];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int s = blockIdx.x;
    const int b = blockIdx.y;
    int64_t first = ranges[2 * b], n = ranges[2 * b + 1];
    int64_t r0 = 0, r1 = 0;                                          // rows [r0, r1) of x
    if (pool_range_ok(first, n, M)) {
        if (mode == 1) {
            if (s == 0) { r0 = first + n - 1; r1 = first + n; }
        } else {
            const int64_t chunk = (n + n_strips - 1) / n_strips;
            r0 = first + min(n, (int64_t)s * chunk);
            r1 = first + min(n, (int64_t)(s + 1) * chunk);
        }
    }
    float acc[NV][8];
#pragma unroll
    for (int i = 0; i < NV; ++i)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[i][e] = 0.f;
    for (int64_t row = r0 + wave; row < r1; row += 4) {
        const uint4* xr = x + row * ld_vec;
        uint4 v[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = lane + 64 * i;
            v[i] = idx < nvec ? xr[idx] : make_uint4(0u, 0u, 0u, 0u);
        }
        float w = 1.0f;
        if (NORM) {
            float ss = 0.f;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                float f[8];
                pool_unpack8(v[i], f);
#pragma unroll
                for (int e = 0; e < 8; ++e) ss = fmaf(f[e], f[e], ss);
            }
            ss = wave_sum(ss);
            w = 1.0f / (sqrtf(ss) * inv_sqrt_d + eps);               // evo_rmsnorm_bf16's factor, bit for bit
        }
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            float f[8];
            pool_unpack8(v[i], f);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[i][e] = NORM ? fmaf(f[e], w, acc[i][e]) : acc[i][e] + f[e];
        }
    }
    // waves (0 + 2) + (1 + 3), then the pair: a fixed order
    if (wave >= 2) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = lane + 64 * i;
            if (idx < nvec) {
                *(f32x4_t*)&red[wave - 2][8 * idx] = f32x4_t{acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
                *(f32x4_t*)&red[wave - 2][8 * idx + 4] = f32x4_t{acc[i][4], acc[i][5], acc[i][6], acc[i][7]};
            }
        }
    }
    __syncthreads();
    if (wave < 2) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = lane + 64 * i;
            if (idx < nvec) {
#pragma unroll
                for (int e = 0; e < 8; ++e) acc[i][e] += red[wave][8 * idx + e];
            }
        }
    }
    __syncthreads();
    if (wave == 1) {
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = lane + 64 * i;
            if (idx < nvec) {
                *(f32x4_t*)&red[0][8 * idx] = f32x4_t{acc[i][0], acc[i][1], acc[i][2], acc[i][3]};
                *(f32x4_t*)&red[0][8 * idx + 4] = f32x4_t{acc[i][4], acc[i][5], acc[i][6], acc[i][7]};
            }
        }
    }
    __syncthreads();
    if (wave == 0) {
        f32x4_t* slab = (f32x4_t*)(ws + ((int64_t)b * n_strips + s) * (int64_t)nvec * 8);
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int idx = lane + 64 * i;
            if (idx < nvec) {
                f32x4_t lo = {acc[i][0] + red[0][8 * idx], acc[i][1] + red[0][8 * idx + 1], acc[i][2] + red[0][8 * idx + 2],
                              acc[i][3] + red[0][8 * idx + 3]};
                f32x4_t hi = {acc[i][4] + red[0][8 * idx + 4], acc[i][5] + red[0][8 * idx + 5], acc[i][6] + red[0][8 * idx + 6],
                              acc[i][7] + red[0][8 * idx + 7]};
                slab[2 * idx] = lo;
                slab[2 * idx + 1] = hi;
            }
        }
    }
}

// One workgroup per (64 columns, sequence): wave w adds slabs w, w + 16, ... in order, the 16 waves' sums meet in LDS in wave order.
__global__ __launch_bounds__(1024) void pool_finish_kernel(const float* __restrict__ ws, const int64_t* __restrict__ ranges, int64_t M,
                                                           int64_t D, int mode, int n_strips, const uint16_t* __restrict__ scale,
                                                           float* __restrict__ out) {
    __shared__ float part[16][64];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int64_t d = (int64_t)blockIdx.x * 64 + lane;
    const int b = blockIdx.y;
    float sum = 0.f;
    if (d < D) {
        const float* p = ws + (int64_t)b * n_strips * D + d;
        for (int s = wave; s < n_strips; s += 16) sum += p[(int64_t)s * D];
    }
    part[wave][lane] = sum;
    __syncthreads();
    if (wave == 0 && d < D) {
        float t = part[0][lane];
        for (int w = 1; w < 16; ++w) t += part[w][lane];
        const int64_t first = ranges[2 * b], n = ranges[2 * b + 1];
        if (!pool_range_ok(first, n, M)) {
            t = __builtin_nanf("");
        } else {
            if (mode == 0) t *= 1.0f / (float)n;
            if (scale) t *= bf_to_f(scale[d]);
        }
        out[(int64_t)b * D + d] = t;
    }
}

extern "C" int evo_pool_rows_bf16(const void* x, int64_t M, int64_t D, int64_t ld, const int64_t* ranges, int64_t B,
                                  const void* scale, float eps, int64_t mode, int64_t n_strips, float* ws, float* out, void* stream) {
    if (!x || !ranges || !ws || !out) return -1;
    if (D <= 0 || D % 8 != 0 || D > EVO_POOL_MAX_D || ld < D || ld % 8 != 0 || M < 1) return -1;
    if (B < 1 || B > 65535 || n_strips < 1 || n_strips > 65535 || (mode != 0 && mode != 1)) return -1;
    const int nvec = (int)(D / 8);
    const float isd = 1.0f / sqrtf((float)D);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)n_strips, (unsigned)B);
#define EVO_POOL_LAUNCH(NV)                                                                                                         \
    do {                                                                                                                            \
        if (scale)                                                                                                                  \
            hipLaunchKernelGGL((pool_strip_kernel<NV, true>), grid, dim3(256), 0, st, (const uint4*)x, M, nvec, ld / 8, ranges,     \
                               (int)mode, (int)n_strips, eps, isd, ws);                                                             \
        else                                                                                                                        \
            hipLaunchKernelGGL((pool_strip_kernel<NV, false>), grid, dim3(256), 0, st, (const uint4*)x, M, nvec, ld / 8, ranges,    \
                               (int)mode, (int)n_strips, eps, isd, ws);                                                             \
    } while (0)
    if (nvec <= 64) EVO_POOL_LAUNCH(1);
    else if (nvec <= 128) EVO_POOL_LAUNCH(2);
    else if (nvec <= 256) EVO_POOL_LAUNCH(4);
    else EVO_POOL_LAUNCH(8);
#undef EVO_POOL_LAUNCH
    int err = evo_launch_status();
    if (err) return err;
    hipLaunchKernelGGL(pool_finish_kernel, dim3((unsigned)((D + 63) / 64), (unsigned)B), dim3(1024), 0, st, ws, ranges, M, D, (int)mode,
                       (int)n_strips, (const uint16_t*)scale, out);
    return evo_launch_status();
}
