// The n-split MFMA weight-streaming kernel, its slice reduction and the host's m-tile dispatch: shared by csrc/gemv.hip (the default
// small-M routing, which picks a form per row count) and csrc/gemv_inv.hip (the row-invariant entries, whose form is a function of the
// layer's shape alone).
#pragma once
#include "gemv_common.h"

typedef float gv_f32x4 __attribute__((ext_vector_type(4)));

// ---- 5 <= M <= 64, N >= 8192: n-split form (round 6).  The k-split form above is bound by L2, not by HBM: every weight fragment (1 KiB per
// wave) pulls MT x fragments of the same size through L2 -- weights + x add up to 6-7 TB/s at every M (4.0 TB/s of weights at 8 rows, 3.4 at
// 16, 2.2 at 32, 1.5 at 64; tools/bench_gemv.py) where hipBLASLt streams 4.2 TB/s at 32-64 rows.  Here a workgroup is WAVES waves, each owning a
// 16-row n tile for the WHOLE K (no partial sums, no reduction), and the x rows of a chunk of KC MFMA steps are staged in LDS once per workgroup and
// read by all its waves as B fragments (ds_read_b128, conflict-free at the padded row pitch): x costs L2 MT / WAVES of the weight bytes
// instead of MT.  K % 256 == 0.
// The weight requests are CONTIGUOUS.  Asked for as the MFMA wants it -- 64 bytes of each of 16 rows that lie K * 2 bytes apart -- a weight fragment
// streams 3.1-3.3 TB/s where 1 KiB contiguous per request runs 4.3-4.4 (profiles/r06_small_m_nsplit_ab.txt; a ring of three fragment sets in flight
// measured 5-8 % SLOWER: the form is not latency-bound, what caps it is the access pattern).  So a request covers RPI = 2 (4) whole row pieces of
// 512 (256) contiguous bytes, the wave parks the chunk in a PRIVATE LDS region in row order and reads its fragments back from there (ds_write_b128 /
// ds_read_b128, both conflict-free at the padded row pitch); the requests of chunk c + 1 (weights and x rows) are in flight while chunk c multiplies.
// SPLITK (N < 8192, the two N = 4,096 layers of a block): blockIdx.y is a slice of the 256-k chunks; the slice's fp32 partial sums go to
// ws [slices][M][N] and skinny_reduce_kernel adds them in slice order (+ bias, + residual, one rounding) -- 64 n groups x 4 slices = a workgroup
// per CU with x still shared four ways, where the k-split form is L2-bound on x (2.1 TB/s at 32 rows).
// GATE (WAVES = 4): the gated MLP's first half [REF stripedhyena/layers.py ParallelGatedMLP: gelu(l1 x) * l2 x] in one launch -- a workgroup's 64 weight rows are
// 32 rows of W1 (waves 0, 1) and the MATCHING 32 rows of W2 (waves 2, 3): one block of the grouped layout (`gate_layout` 1: HipOps.pack_gate_weights), or rows
// c .. c + 31 and I + c .. of the plain [W1; W2] (2).  Waves 2, 3 hand their z2 tiles over through LDS; z1, z2 are rounded to bf16 (the dense layer's outputs),
// the gate is evaluated in fp32 and rounded once: bit for bit the dense layer + evo_gelu_gate_bf16.  N = 2 I, y = a [M, I].
// SLICE256 (SPLITK only; csrc/gemv_inv.hip): the slices are cut in units of 256 k whatever the chunk length, so a slice's k range -- and with it every
// partial sum -- does not depend on MT.  (The default's cut is in chunks of KC steps: at K = 11,008 it falls at k = 2,560 with MT <= 2 and at 2,688 above.)
template <int MT, int WAVES, bool SPLITK = false, bool GATE = false, bool SLICE256 = false>
__global__ __launch_bounds__(64 * WAVES) void skinny_nw_kernel(const uint4* __restrict__ x, const uint4* __restrict__ w,
                                                               const uint16_t* __restrict__ bias, const uint16_t* res,
                                                               uint16_t* y, int M, int N, int nvec, float* __restrict__ ws = nullptr,
                                                               int gate_layout = 0) {   // res may alias y
    static_assert(!GATE || (WAVES == 4 && !SPLITK), "a gated workgroup is one 32 + 32 row block");
    constexpr int KC = MT <= 2 ? 8 : 4;                          // MFMA steps (32 k) per chunk
    constexpr int ROWB = KC * 64 + 16;                           // LDS bytes per row of a chunk (+ 16 pad: b128 accesses at this pitch touch all banks)
    constexpr int PPR = KC * 4;                                  // 16-byte pieces per row of a chunk
    constexpr int RPI = 64 / PPR;                                // weight rows per request
    constexpr int XL = (MT * 16 * PPR + 64 * WAVES - 1) / (64 * WAVES);   // x pieces per thread and chunk
    __shared__ __attribute__((aligned(16))) unsigned char xs[2][MT * 16 * ROWB];
    __shared__ __attribute__((aligned(16))) unsigned char wsm[WAVES][16 * ROWB];
    typedef unsigned int sn_u32x4 __attribute__((ext_vector_type(4)));   // (native vectors: loop-carried uint4 arrays end up in scratch memory)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, kb = lane >> 4;
    const int n0 = GATE && gate_layout == 2 ? (wave < 2 ? blockIdx.x * 32 + wave * 16 : (N >> 1) + blockIdx.x * 32 + (wave - 2) * 16)
                                            : (blockIdx.x * WAVES + wave) * 16;
    const int n_chunk_all = nvec / PPR;
    static_assert(!SLICE256 || SPLITK, "SLICE256 says how a split over K is cut");
    constexpr int CPU = 8 / KC;                                  // chunks per 256 k
    const int n_cut = SLICE256 ? n_chunk_all / CPU : n_chunk_all, cut = SLICE256 ? CPU : 1;
    const int c_first = SPLITK ? (int)((int64_t)n_cut * blockIdx.y / gridDim.y) * cut : 0;
    const int n_chunk = SPLITK ? (int)((int64_t)n_cut * (blockIdx.y + 1) / gridDim.y) * cut : n_chunk_all;   // chunks [c_first, n_chunk) are this workgroup's
    // request i of a chunk: weight row n0 + RPI i + lane / PPR, piece lane % PPR
    const int q_row = lane / PPR, q_piece = lane % PPR;
    const sn_u32x4* wq[KC];
#pragma unroll
    for (int i = 0; i < KC; ++i) {
        const int row = n0 + RPI * i + q_row < N ? n0 + RPI * i + q_row : N - 1;
        wq[i] = (const sn_u32x4*)(w + (int64_t)row * nvec + q_piece);
    }
    unsigned char* wmine = wsm[wave];
    const int w_st = q_row * ROWB + q_piece * 16;               // + RPI * i * ROWB
    const int f_rd = r16 * ROWB + kb * 16;                       // + u * 64
    gv_f32x4 acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = gv_f32x4{0.f, 0.f, 0.f, 0.f};
    sn_u32x4 xr[XL], wr[KC];
#define SW_X_LOAD(C)                                                                                          \
    _Pragma("unroll") for (int i_ = 0; i_ < XL; ++i_) {                                                       \
        const int pidx_ = tid + i_ * 64 * WAVES;                                                              \
        int row_ = pidx_ / PPR;                                                                               \
        row_ = row_ < M ? row_ : M - 1;              /* rows past M (and pieces past the chunk) re-read a valid row: never stored */ \
        xr[i_] = *(const sn_u32x4*)(x + (int64_t)row_ * nvec + (C) * PPR + (pidx_ % PPR));                    \
    }
#define SW_X_STORE(BUF)                                                                                       \
    _Pragma("unroll") for (int i_ = 0; i_ < XL; ++i_) {                                                       \
        const int pidx_ = tid + i_ * 64 * WAVES;                                                              \
        if (pidx_ < MT * 16 * PPR) *(sn_u32x4*)(xs[BUF] + (pidx_ / PPR) * ROWB + (pidx_ % PPR) * 16) = xr[i_]; \
    }
#define SW_W_LOAD(C) _Pragma("unroll") for (int i_ = 0; i_ < KC; ++i_) wr[i_] = __builtin_nontemporal_load(wq[i_] + (C) * PPR);
#define SW_W_STORE() _Pragma("unroll") for (int i_ = 0; i_ < KC; ++i_) *(sn_u32x4*)(wmine + w_st + RPI * i_ * ROWB) = wr[i_];
    auto mul = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < KC; ++u) {
            const uint4 wv = *(const uint4*)(wmine + f_rd + u * 64);
#pragma unroll
            for (int t = 0; t < MT; ++t) {
                const uint4 xv = *(const uint4*)(xs[buf] + (16 * t + r16) * ROWB + u * 64 + kb * 16);
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, wv), __builtin_bit_cast(bf16x8_t, xv), acc[t], 0, 0, 0);
            }
        }
    };
    SW_X_LOAD(c_first);
    SW_W_LOAD(c_first);
    SW_X_STORE(c_first & 1);
    SW_W_STORE();
    __syncthreads();
    for (int c = c_first; c < n_chunk; ++c) {
        const int buf = c & 1;
        if (c + 1 < n_chunk) { SW_X_LOAD(c + 1); SW_W_LOAD(c + 1); }
        mul(buf);
        // no barrier here: x buffer buf ^ 1 has been free since the last barrier, and the weight region is the wave's own -- its stores follow its reads
        // in program order (same LDS array: the compiler keeps the order, the LDS unit executes a wave's accesses in order)
        if (c + 1 < n_chunk) { SW_X_STORE(buf ^ 1); SW_W_STORE(); }
        __syncthreads();
    }
#undef SW_X_LOAD
#undef SW_X_STORE
#undef SW_W_LOAD
#undef SW_W_STORE
    if constexpr (GATE) {
        // (the last barrier of the chunk loop is behind every wave's last fragment read: xs is free)
        float* ex = (float*)&xs[0][0];                           // [2 waves][MT][64 lanes] x 16 B <= 4 KiB
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
            if (m < M && n0 + 4 * kb < N) *(gv_f32x4*)(wsl + (int64_t)m * N + n0 + 4 * kb) = acc[t];     // (N % 4 == 0 on this path)
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

// y [M, N] = sum over slices of ws [slices][M][N] (in slice order: deterministic) + bias + residual, one rounding; a thread owns four columns
// (static: both files that include this header launch their own copy)
static __global__ __launch_bounds__(256) void skinny_reduce_kernel(const float* __restrict__ ws, const uint16_t* __restrict__ bias, const uint16_t* res,
                                                            uint16_t* y, int M, int N, int slices) {   // res may alias y
    const int64_t q = (int64_t)blockIdx.x * 256 + threadIdx.x, total = (int64_t)M * N / 4;
    if (q >= total) return;
    const int64_t e = q * 4;
    const int n = (int)(e % N);
    gv_f32x4 a = *(const gv_f32x4*)(ws + e);
    for (int sl = 1; sl < slices; ++sl) a += *(const gv_f32x4*)(ws + (int64_t)sl * M * N + e);
    float o[4] = {a[0], a[1], a[2], a[3]};
    if (bias) { const uint2 b = *(const uint2*)(bias + n); o[0] += bf_lo(b.x); o[1] += bf_hi(b.x); o[2] += bf_lo(b.y); o[3] += bf_hi(b.y); }
    if (res) { const uint2 r = *(const uint2*)(res + e); o[0] += bf_lo(r.x); o[1] += bf_hi(r.x); o[2] += bf_lo(r.y); o[3] += bf_hi(r.y); }
    uint2 out;
    out.x = pack_bf2(o[0], o[1]);
    out.y = pack_bf2(o[2], o[3]);
    *(uint2*)(y + e) = out;
}

// host side: compile-time constants from run-time row counts, as f(gv_int<V>) (for_m, for_m_stage: gemv_common.h).  for_mt: the skinny
// MFMA kernels' MT (m tiles of 16 batch rows, M <= 64).
template <class F>
static void for_mt(int64_t M, F f) {
    if (M <= 16) f(gv_int<1>{}); else if (M <= 32) f(gv_int<2>{}); else if (M <= 48) f(gv_int<3>{}); else f(gv_int<4>{});
}
