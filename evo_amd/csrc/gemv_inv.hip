// Row-invariant weight-streaming dense layers: y[M,N] = x[M,K] . W[N,K]^T (+ bias) (+ residual) and the gated MLP's first
// half for 1 <= M <= 64 batch rows, where every output element sees ONE fixed sequence of operations whatever M is -- row i of an M-row call is bit
// for bit the one-row call on row i.  csrc/gemv.hip picks a form per row count (dot2 up to 4 rows, k-split MFMA, n-split MFMA, split over K from 17
// rows), and each form sums K in another order; here the form, the partition of K and the reduction tree are functions of (N, K) alone:
//   N >= 8192                 skinny_nw_kernel<MT, 2 | 3 | 4 waves by N>: a wave owns a 16-row n tile for the whole K, 32 k per MFMA in k order
//   N <  8192                 skinny_nw_kernel<MT, 4 (2 below N = 2048), SPLITK, SLICE256>: `rowinv_slices(N, K)` slices of whole 256-k units, fp32
//                             partial sums through the caller's workspace, skinny_reduce_kernel adds them in slice order (+ bias, + residual, one rounding)
//   gate                      skinny_nw_kernel<MT, 4, GATE>, either weight layout
// The batch rows are the N side of v_mfma_f32_16x16x32_bf16: an output column's 32-term sums read that column's x row only, so neither the values
// (NaN included) nor the number of the other rows reach it.  Only MT -- the m tiles of 16 rows a weight fragment meets -- follows M; it changes how
// many accumulators a wave carries and how long a staged chunk is (8 or 4 MFMA steps), never the order of the steps of one accumulator.
// Shape contract (anything else: -1, there is no second form to fall back to): K % 256 == 0; N % 64 == 0; for the gate I % 32 == 0.
// Entry points: include/evo_mi355x.h.
#include "skinny_nw.h"
#include "../../include/evo_mi355x.h"

// slices of a narrow layer's K: a workgroup per CU where the layer allows it, at most 8, at least one 256-k unit each -- from (N, K) only
static int64_t rowinv_slices(int64_t N, int64_t K) {
    const int64_t groups = N / (N < 2048 ? 32 : 64);
    int64_t slices = (256 + groups - 1) / groups;
    if (slices > K / 256) slices = K / 256;
    return slices > 8 ? 8 : slices;
}

extern "C" int evo_linear_rowinv_bf16(const void* x, const void* w, const void* bias, const void* residual, void* y,
                                      int64_t M, int64_t N, int64_t K, void* ws, int64_t ws_bytes, void* stream) {
    if (M < 1 || M > 64 || N <= 0 || K <= 0 || K % 256 != 0 || N % 64 != 0 || N > 0x7fffffff - 64 || K > 0x7fffffff) return -1;
    hipStream_t s = (hipStream_t)stream;
    const uint4 *xp = (const uint4*)x, *wp = (const uint4*)w;
    const uint16_t *bp = (const uint16_t*)bias, *rp = (const uint16_t*)residual;
    uint16_t* yp = (uint16_t*)y;
    const int nvec = (int)(K / 8);
    if (N >= 8192) {
        const auto launch = [&](auto mt, auto waves) {
            constexpr int WV = decltype(waves)::value;
            hipLaunchKernelGGL((skinny_nw_kernel<decltype(mt)::value, WV>), dim3((unsigned)((N + 16 * WV - 1) / (16 * WV))), dim3(64 * WV), 0, s, xp, wp, bp, rp,
                               yp, (int)M, (int)N, nvec);
        };
        for_mt(M, [&](auto mt) {
            if (N >= 256 * 64) launch(mt, gv_int<4>{}); else if (N >= 256 * 48) launch(mt, gv_int<3>{}); else launch(mt, gv_int<2>{});
        });
        return evo_launch_status();
    }
    const int64_t slices = rowinv_slices(N, K);
    if (!ws || ((uintptr_t)ws & 15) != 0 || ws_bytes < slices * M * N * 4) return -1;
    const auto launch = [&](auto mt, auto waves) {
        constexpr int WV = decltype(waves)::value;
        hipLaunchKernelGGL((skinny_nw_kernel<decltype(mt)::value, WV, true, false, true>), dim3((unsigned)(N / (16 * WV)), (unsigned)slices), dim3(64 * WV), 0, s,
                           xp, wp, (const uint16_t*)nullptr, (const uint16_t*)nullptr, (uint16_t*)nullptr, (int)M, (int)N, nvec, (float*)ws);
    };
    for_mt(M, [&](auto mt) {
        if (N < 2048) launch(mt, gv_int<2>{}); else launch(mt, gv_int<4>{});
    });
    hipLaunchKernelGGL(skinny_reduce_kernel, dim3((unsigned)((M * N / 4 + 255) / 256)), dim3(256), 0, s, (const float*)ws, bp, rp, yp, (int)M, (int)N, (int)slices);
    return evo_launch_status();
}

extern "C" int evo_mlp_gate_rowinv_bf16(const void* x, const void* w12, void* a, int64_t M, int64_t I, int64_t K, int64_t grouped,
                                        void* stream) {
    if (M < 1 || M > 64 || I <= 0 || I % 32 != 0 || K <= 0 || K % 256 != 0 || I > 0x1fffffff || K > 0x7fffffff) return -1;
    hipStream_t s = (hipStream_t)stream;
    for_mt(M, [&](auto mt) {
        hipLaunchKernelGGL((skinny_nw_kernel<decltype(mt)::value, 4, false, true>), dim3((unsigned)(I / 32)), dim3(256), 0, s, (const uint4*)x, (const uint4*)w12,
                           (const uint16_t*)nullptr, (const uint16_t*)nullptr, (uint16_t*)a, (int)M, (int)(2 * I), (int)(K / 8), (float*)nullptr, grouped ? 1 : 2);
    });
    return evo_launch_status();
}
