// Weight-streaming dense layers of a decode step on FP8 (OCP e4m3fn) WEIGHTS at 5-64 batch rows (include/evo_mi355x.h, ABI 20; DESIGN.md
// section 28): skinny_nw_kernel's three forms (csrc/skinny_nw.h: n-split, SPLITK, GATE) with one byte per weight to stream.
//
// The record is csrc/gemv_fp8.hip's: data [N, K] bytes row-major, scale [N] f32 powers of two (evo_w_quant_fp8).  As in the bf16 sibling a
// wave owns a 16-row n tile, the x rows of a chunk are staged once per workgroup in LDS, and the weights are requested as CONTIGUOUS row
// pieces -- here 256 (MT <= 2) or 128 (MT >= 3) bytes of each of 4 (8) rows per request -- and parked, AS BYTES, in a wave-private LDS
// region in row order.  A lane reads its 8 weights of an MFMA step back with one ds_read_b64 and converts them with four
// v_cvt_scalef32_pk_bf16_fp8 (scale operand 1.0: the plain, exact conversion); the converted A fragment is shared by the MT m tiles.
// The sums are taken in the byte domain; the row's scale multiplies the fp32 sum ONCE per output element (per partial sum under SPLITK: a
// power of two, exact), before bias, residual or gate.
// With half the bytes per chunk a wave has half the bf16 form's bytes in flight, so the weight requests run TWO chunks ahead (a ring of
// two register sets; the chunk loop is unrolled by two so that the ring index is static), x one chunk ahead as in the sibling.  Within a
// step the x requests go out BEFORE the weight requests of chunk c + 2: vmcnt retires in order, and the wait in front of the LDS stores
// of chunk c + 1 then leaves the youngest weight requests in flight.
// Slices (SPLITK) are cut in units of 256 k whatever the chunk length.
#include "skinny_nw.h"
#include "fp8_common.h"
#include "../../include/evo_mi355x.h"

__device__ __forceinline__ uint32_t sw8_pair(uint32_t d, bool hi) {     // bytes (0, 1) or (2, 3) of d -> packed bf16 pair, exact
    return hi ? __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d, 1.0f, true))
              : __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d, 1.0f, false));
}

template <int MT, int WAVES, bool SPLITK = false, bool GATE = false>
__global__ __launch_bounds__(64 * WAVES) void skinny_w8_kernel(const uint4* __restrict__ x, const unsigned char* __restrict__ w,
                                                               const float* __restrict__ wscale, const uint16_t* __restrict__ bias,
                                                               const uint16_t* res, uint16_t* y, int M, int N, int K,
                                                               float* __restrict__ ws, int gate_layout) {   // res may alias y
    static_assert(!GATE || (WAVES == 4 && !SPLITK), "a gated workgroup is one 32 + 32 row block");
    constexpr int KC = MT <= 2 ? 8 : 4;                          // MFMA steps (32 k) per chunk
    constexpr int XROWB = KC * 64 + 16;                          // LDS bytes per x row of a chunk (+ 16 pad, as the sibling)
    constexpr int WROWB = KC * 32 + 16;                          // LDS bytes per weight row of a chunk
    constexpr int XPPR = KC * 4;                                 // 16-byte pieces per x row of a chunk
    constexpr int WPPR = KC * 2;                                 // 16-byte pieces per weight row of a chunk
    constexpr int RPI = 64 / WPPR;                               // weight rows per request
    constexpr int WR = 16 / RPI;                                 // weight requests per chunk
    constexpr int XL = (MT * 16 * XPPR + 64 * WAVES - 1) / (64 * WAVES);   // x pieces per thread and chunk
    constexpr int CPU = 8 / KC;                                  // chunks per 256 k
    __shared__ __attribute__((aligned(16))) unsigned char xs[2][MT * 16 * XROWB];
    __shared__ __attribute__((aligned(16))) unsigned char wsm[WAVES][16 * WROWB];
    typedef unsigned int sn_u32x4 __attribute__((ext_vector_type(4)));
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, kb = lane >> 4;
    const int n0 = GATE && gate_layout == 2 ? (wave < 2 ? blockIdx.x * 32 + wave * 16 : (N >> 1) + blockIdx.x * 32 + (wave - 2) * 16)
                                            : (blockIdx.x * WAVES + wave) * 16;
    const int nvec = K >> 3;                                     // 16-byte pieces per x row
    const int units = K >> 8;
    const int c0 = SPLITK ? (int)((int64_t)units * blockIdx.y / gridDim.y) * CPU : 0;
    const int nc = (SPLITK ? (int)((int64_t)units * (blockIdx.y + 1) / gridDim.y) * CPU : units * CPU) - c0;   // chunks c0 .. c0 + nc - 1
    // request i of a chunk: weight row n0 + RPI i + lane / WPPR, piece lane % WPPR
    const int q_row = lane / WPPR, q_piece = lane % WPPR;
    const sn_u32x4* wq[WR];
#pragma unroll
    for (int i = 0; i < WR; ++i) {
        const int row = n0 + RPI * i + q_row < N ? n0 + RPI * i + q_row : N - 1;      // rows past N re-read the last row: never stored
        wq[i] = (const sn_u32x4*)(w + (int64_t)row * K) + q_piece;
    }
    // this lane's four output features n0 + 4 kb + r: their scales, requested ahead of the stream
    float sc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) sc[r] = wscale[n0 + 4 * kb + r < N ? n0 + 4 * kb + r : N - 1];
    unsigned char* wmine = wsm[wave];
    const int w_st = q_row * WROWB + q_piece * 16;              // + RPI * i * WROWB
    const int f_rd = r16 * WROWB + kb * 8;                       // + u * 32
    gv_f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = gv_f32x4{0.f, 0.f, 0.f, 0.f};
    sn_u32x4 xr[XL], wr[2][WR];
#define SW_X_LOAD(C)                                                                                          \
    _Pragma("unroll") for (int i_ = 0; i_ < XL; ++i_) {                                                       \
        const int pidx_ = tid + i_ * 64 * WAVES;                                                              \
        int row_ = pidx_ / XPPR;                                                                              \
        row_ = row_ < M ? row_ : M - 1;              /* rows past M (and pieces past the chunk) re-read a valid row: never stored */ \
        xr[i_] = *(const sn_u32x4*)(x + (int64_t)row_ * nvec + (C) * XPPR + (pidx_ % XPPR));                  \
    }
#define SW_X_STORE(BUF)                                                                                       \
    _Pragma("unroll") for (int i_ = 0; i_ < XL; ++i_) {                                                       \
        const int pidx_ = tid + i_ * 64 * WAVES;                                                              \
        if (pidx_ < MT * 16 * XPPR) *(sn_u32x4*)(xs[BUF] + (pidx_ / XPPR) * XROWB + (pidx_ % XPPR) * 16) = xr[i_]; \
    }
#define SW_W_LOAD(S, C) _Pragma("unroll") for (int i_ = 0; i_ < WR; ++i_) wr[S][i_] = __builtin_nontemporal_load(wq[i_] + (C) * WPPR);
#define SW_W_STORE(S) _Pragma("unroll") for (int i_ = 0; i_ < WR; ++i_) *(sn_u32x4*)(wmine + w_st + RPI * i_ * WROWB) = wr[S][i_];
    auto mul = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < KC; ++u) {
            const uint2 d = *(const uint2*)(wmine + f_rd + u * 32);
            const uint4 wv = make_uint4(sw8_pair(d.x, false), sw8_pair(d.x, true), sw8_pair(d.y, false), sw8_pair(d.y, true));
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                const uint4 xv = *(const uint4*)(xs[buf] + (16 * t + r16) * XROWB + u * 64 + kb * 16);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wv), __builtin_bit_cast(bf16x8_t, xv), acc[t], 0, 0, 0);
            }
        }
    };
    // step j (S = j & 1): LDS holds chunk j (x in xs[S], weights in the wave's region), wr[S ^ 1] is chunk j + 1, in flight or landed
#define SW_STEP(J, S)                                                                                         \
    {                                                                                                         \
        if ((J) + 1 < nc) { SW_X_LOAD(c0 + (J) + 1); }                                                        \
        if ((J) + 2 < nc) { SW_W_LOAD(S, c0 + (J) + 2); }                                                     \
        mul(S);                                                                                               \
        /* no barrier here: x buffer S ^ 1 has been free since the last barrier, and the weight region is the wave's own (see the sibling) */ \
        if ((J) + 1 < nc) { SW_X_STORE((S) ^ 1); SW_W_STORE((S) ^ 1); }                                       \
        __syncthreads();                                                                                      \
    }
    SW_X_LOAD(c0);
    SW_W_LOAD(0, c0);
    if (nc > 1) { SW_W_LOAD(1, c0 + 1); }
    SW_X_STORE(0);
    SW_W_STORE(0);
    __syncthreads();
    for (int j = 0; j < nc; j += 2) {                            // (nc is workgroup-uniform: every wave meets every barrier)
        SW_STEP(j, 0);
        if (j + 1 < nc) SW_STEP(j + 1, 1);
    }
#undef SW_STEP
#undef SW_X_LOAD
#undef SW_X_STORE
#undef SW_W_LOAD
#undef SW_W_STORE
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[t][r] *= sc[r];
    if constexpr (GATE) {
        // (the last barrier of the chunk loop is behind every wave's last fragment read: xs is free)
        float* ex = (float*)&xs[0][0];                           // [2 waves][MT][64 lanes] x 16 B <= 8 KiB
        if (wave >= 2) {
#pragma unroll
            for (int t = 0; t < MT; ++t) *(gv_f32x4*)(ex + (((wave - 2) * MT + t) * 64 + lane) * 4) = acc[t];
        }
        __syncthreads();
        if (wave < 2) {
            const int I_ = N >> 1;
            const int col0 = blockIdx.x * 32 + wave * 16 + 4 * kb;           // this lane's four gated columns
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                const gv_f32x4 z2 = *(const gv_f32x4*)(ex + ((wave * MT + t) * 64 + lane) * 4);
                const int m = 16 * t + r16;
                if (m < M && col0 < I_) {
                    const f32x2_t ua = {round_bf(acc[t][0]), round_bf(acc[t][1])}, ga = {round_bf(z2[0]), round_bf(z2[1])};
                    const f32x2_t ub = {round_bf(acc[t][2]), round_bf(acc[t][3])}, gb = {round_bf(z2[2]), round_bf(z2[3])};
                    const f32x2_t oa = gelu_gate2(ua, ga), ob = gelu_gate2(ub, gb);
                    uint2 o;
                    o.x = pack_bf2(oa[0], oa[1]);
                    o.y = pack_bf2(ob[0], ob[1]);
                    *(uint2*)(y + (int64_t)m * I_ + col0) = o;               // (I % 32 == 0: whole groups of four)
                }
            }
        }
        return;
    }
    if constexpr (SPLITK) {
        float* wsl = ws + (int64_t)blockIdx.y * M * N;
#pragma unroll
        for (int t = 0; t < MT; ++t) {
            const int m = 16 * t + r16;
            if (m < M && n0 + 4 * kb < N) *(gv_f32x4*)(wsl + (int64_t)m * N + n0 + 4 * kb) = acc[t];     // (N % 64 == 0 on this path)
        }
        return;
    }
#pragma unroll
    for (int t = 0; t < MT; ++t) {
        const int m = 16 * t + r16;
        if (m < M) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + 4 * kb + r;
                if (n < N) {
                    float o = acc[t][r] + (bias ? bf_to_f(bias[n]) : 0.f);
                    if (res) o += bf_to_f(res[(int64_t)m * N + n]);
                    y[(int64_t)m * N + n] = f_to_bf(o);
                }
            }
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
static bool sw8_aligned(const void* p, uintptr_t a) { return p && ((uintptr_t)p & (a - 1)) == 0; }
static bool sw8_aligned_or_null(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
static bool sw8_common_ok(const void* x, const void* w_data, const float* w_scale, const void* y, int64_t M, int64_t K) {
    return sw8_aligned(x, 16) && sw8_aligned(w_data, 16) && sw8_aligned(w_scale, 4) && sw8_aligned(y, 16) && M >= 5 && M <= 64 &&
           K >= 256 && K % 256 == 0 && K <= 0x7fffff00;
}

extern "C" int evo_linear_skinny_w8(const void* x, const void* w_data, const float* w_scale, const void* bias, const void* residual,
                                    void* y, int64_t M, int64_t N, int64_t K, void* ws, int64_t ws_bytes, void* stream) {
    if (!sw8_common_ok(x, w_data, w_scale, y, M, K) || !sw8_aligned_or_null(bias, 16) || !sw8_aligned_or_null(residual, 16) ||
        !sw8_aligned_or_null(ws, 16) || N < 1 || N > 0x7fffffff - 64 || ws_bytes < 0)
        return -1;
    hipStream_t s = (hipStream_t)stream;
    const uint4* xp = (const uint4*)x;
    const unsigned char* wp = (const unsigned char*)w_data;
    const uint16_t *bp = (const uint16_t*)bias, *rp = (const uint16_t*)residual;
    uint16_t* yp = (uint16_t*)y;
    // narrow layers (N < 8192: out_filter_dense / out_proj / l3 of a 7B block) with a workspace from the caller: a split over K across
    // workgroups, the slice count by evo_linear_small_m_bf16's rule -- a workgroup per CU, at most 8 slices, a 256-k unit or more each
    if (ws && N < 8192 && N % 64 == 0) {
        int64_t slices = (256 + N / 64 - 1) / (N / 64);
        if (slices > K / 256) slices = K / 256;
        if (slices > 8) slices = 8;
        if (slices >= 2 && ws_bytes >= slices * M * N * 4) {
            const dim3 grid((unsigned)(N / 64), (unsigned)slices);
            for_mt(M, [&](auto mt) {
                hipLaunchKernelGGL((skinny_w8_kernel<decltype(mt)::value, 4, true>), grid, dim3(256), 0, s, xp, wp, w_scale, (const uint16_t*)nullptr,
                                   (const uint16_t*)nullptr, (uint16_t*)nullptr, (int)M, (int)N, (int)K, (float*)ws, 0);
            });
            hipLaunchKernelGGL(skinny_reduce_kernel, dim3((unsigned)((M * N / 4 + 255) / 256)), dim3(256), 0, s, (const float*)ws, bp, rp, yp, (int)M,
                               (int)N, (int)slices);
            return evo_launch_status();
        }
    }
    // n-split form, whole K per wave; WAVES n tiles per workgroup = a workgroup or more per CU where N allows (any N: the last tile is clamped)
    const auto launch = [&](auto mt, auto waves) {
        constexpr int WV = decltype(waves)::value;
        hipLaunchKernelGGL((skinny_w8_kernel<decltype(mt)::value, WV>), dim3((unsigned)((N + 16 * WV - 1) / (16 * WV))), dim3(64 * WV), 0, s, xp, wp, w_scale,
                           bp, rp, yp, (int)M, (int)N, (int)K, (float*)nullptr, 0);
    };
    for_mt(M, [&](auto mt) {
        if (N >= 256 * 64) launch(mt, gv_int<4>{}); else if (N >= 256 * 48) launch(mt, gv_int<3>{}); else launch(mt, gv_int<2>{});
    });
    return evo_launch_status();
}

extern "C" int evo_mlp_gate_skinny_w8(const void* x, const void* w12_data, const float* w12_scale, void* a, int64_t M, int64_t I,
                                      int64_t K, int64_t grouped, void* stream) {
    if (!sw8_common_ok(x, w12_data, w12_scale, a, M, K) || I < 32 || I % 32 != 0 || I > 0x1fffffff) return -1;
    for_mt(M, [&](auto mt) {
        hipLaunchKernelGGL((skinny_w8_kernel<decltype(mt)::value, 4, false, true>), dim3((unsigned)(I / 32)), dim3(256), 0, (hipStream_t)stream,
                           (const uint4*)x, (const unsigned char*)w12_data, w12_scale, (const uint16_t*)nullptr, (const uint16_t*)nullptr,
                           (uint16_t*)a, (int)M, (int)(2 * I), (int)K, (float*)nullptr, grouped ? 1 : 2);
    });
    return evo_launch_status();
}
