// Weight-streaming dense layers of a decode step on FP8 (OCP e4m3fn) WEIGHTS, 1-8 batch rows (include/evo_mi355x.h, ABI 20; DESIGN.md
// section 22): the four dot2 kernels of csrc/gemv.hip with half the bytes to stream, and the kernel that quantises a weight.
//
// THE RULE is the KV cache's (fp8_common.h) with a weight row -- the K values of one output feature n -- in place of a cache row: bytes
// RNE_e4m3fn(W[n, k] 2^-e) and one f32 scale 2^e per row.  Layout: data [N, K] bytes row-major, scale [N] f32, K % 16 == 0.
//
// A lane's 16-byte non-temporal load is 16 weights = weight vector v of the row; it meets x's vectors 2 v and 2 v + 1 (8 bf16 each).
// v_cvt_scalef32_pk_bf16_fp8 (scale operand 1.0: the conversion is then the plain, exact one) turns two bytes into the packed bf16 pair
// v_dot2c_f32_bf16 takes: 8 conversions per 16 weights, shared by the M batch rows, then the bf16 kernels' 8 M dot2.  The sums are
// taken in the byte domain; the row's scale multiplies the reduced fp32 sum ONCE per output element (a power of two: exact), before
// bias, residual, gate or Hyena step.  Everything around the stream -- which wave owns which rows, SPLIT, the LDS staging of the
// normalised rows at K = 4096, the epilogues -- is the bf16 sibling's.
#include "gemv_common.h"
#include "fp8_common.h"
#include "../../include/evo_mi355x.h"

// ---- evo_w_quant_fp8: a workgroup per weight row.  Sweep 1 takes the row maximum (15-bit magnitudes: an integer maximum), sweep 2
// re-reads the row (at most a few tens of KiB, just fetched: L2) and stores the bytes -- one pass over the weight in HBM.
__global__ __launch_bounds__(256) void w_quant_fp8_kernel(const uint4* __restrict__ w, uint2* __restrict__ data, float* __restrict__ scale,
                                                          int nvec8) {
    __shared__ uint32_t wmax[4];
    const int64_t n = blockIdx.x;
    const uint4* row = w + n * nvec8;
    uint32_t m = 0;
    for (int v = threadIdx.x; v < nvec8; v += 256) m = max(m, fp8_max15(row[v]));
    m = fp8_group_max<16>(m);
    m = max(m, (uint32_t)__shfl_xor((int)m, 16, 64));
    m = max(m, (uint32_t)__shfl_xor((int)m, 32, 64));
    if ((threadIdx.x & 63) == 0) wmax[threadIdx.x >> 6] = m;
    __syncthreads();
    const int e = fp8_row_exponent(max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3])));
    const float inv = fp8_pow2(-e);
    uint2* drow = data + n * nvec8;
    for (int v = threadIdx.x; v < nvec8; v += 256) drow[v] = fp8_quant8(row[v], inv);
    if (threadIdx.x == 0) scale[n] = fp8_pow2(e);
}

// ---- the stream ------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t w8_pair(uint32_t d, bool hi) {      // bytes (0, 1) or (2, 3) of d -> packed bf16 pair, exact
    return hi ? __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d, 1.0f, true))
              : __builtin_bit_cast(uint32_t, __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(d, 1.0f, false));
}
// weight vector v of R rows against x's vectors 2 v, 2 v + 1 of the M batch rows; xf(m, j) = vector j (8 bf16) of batch row m
__device__ __forceinline__ uint4 w8_lo(const uint4& q) {
    return make_uint4(w8_pair(q.x, false), w8_pair(q.x, true), w8_pair(q.y, false), w8_pair(q.y, true));
}
__device__ __forceinline__ uint4 w8_hi(const uint4& q) {
    return make_uint4(w8_pair(q.z, false), w8_pair(q.z, true), w8_pair(q.w, false), w8_pair(q.w, true));
}
// Every weight is converted once and every x vector fetched once; one of the two waits in registers for the other.  HOLD_X: the
// slice's x (8 M registers), the rows converted one at a time; otherwise the converted rows (8 R), x one batch row at a time.  Either
// way acc[r][m] takes the row's low half, then its high half: the choice moves registers, never a bit.
template <int M, int R, bool HOLD_X, class XF>
__device__ __forceinline__ void w8_slice(const uint4 (&wq)[R], int v, const XF& xf, float (&acc)[R][M]) {
    if constexpr (HOLD_X) {
        uint4 x0[M], x1[M];
#pragma unroll
        for (int m = 0; m < M; ++m) { x0[m] = xf(m, 2 * v); x1[m] = xf(m, 2 * v + 1); }
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint4 wl = w8_lo(wq[r]), wh = w8_hi(wq[r]);
#pragma unroll
            for (int m = 0; m < M; ++m) acc[r][m] = dot8(wh, x1[m], dot8(wl, x0[m], acc[r][m]));
        }
    } else {
        uint4 wl[R], wh[R];
#pragma unroll
        for (int r = 0; r < R; ++r) { wl[r] = w8_lo(wq[r]); wh[r] = w8_hi(wq[r]); }
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const uint4 x0 = xf(m, 2 * v), x1 = xf(m, 2 * v + 1);
#pragma unroll
            for (int r = 0; r < R; ++r) acc[r][m] = dot8(wh[r], x1, dot8(wl[r], x0, acc[r][m]));
        }
    }
}
// this lane's weight vectors v, v + ST, ... < nv of its wave's R rows: two slices per trip (2 R weight loads in flight), as gemv_kernel
template <int M, int R, bool HOLD_X, class XF>
__device__ __forceinline__ void w8_stream(const uint4* const (&wrow)[R], int nv, int v, int ST, const XF& xf, float (&acc)[R][M]) {
#pragma unroll 1                                             // (the trip is the unrolling: two slices in flight, no more registers)
    for (; v + ST < nv; v += 2 * ST) {
        uint4 w0[R], w1[R];
#pragma unroll
        for (int r = 0; r < R; ++r) { w0[r] = ld_stream(wrow[r] + v); w1[r] = ld_stream(wrow[r] + v + ST); }
        w8_slice<M, R, HOLD_X>(w0, v, xf, acc);
        w8_slice<M, R, HOLD_X>(w1, v + ST, xf, acc);
    }
    for (; v < nv; v += ST) {
        uint4 w0[R];
#pragma unroll
        for (int r = 0; r < R; ++r) w0[r] = ld_stream(wrow[r] + v);
        w8_slice<M, R, HOLD_X>(w0, v, xf, acc);
    }
}

// ---- x as the norm-folding kernels see it.  NORM && !STAGE: every wave reduces sum(x^2) of every row itself and rebuilds the normalised
// slices in registers (any K, 1-4 rows).  STAGE (K = 4096): rows normalised once into LDS (gemv_common.h).  Bit for bit the row
// evo_rmsnorm_bf16 would have stored, either way.
template <int M, bool NORM, bool STAGE>
struct W8X {
    const uint4* x; const uint4* scale; int nvec8; float inv[M];
    __device__ __forceinline__ uint4 operator()(int m, int j) const {
        if constexpr (STAGE) return gv_xn[m * nvec8 + j];
        const uint4 xv = x[(int64_t)m * nvec8 + j];
        if constexpr (!NORM) return xv; else return gv_norm8(xv, scale[j], inv[m]);
    }
};
// STAGE: a K = 4096 row is 256 weight vectors = four per lane.  `issue()` requests the first two of every row (2 R loads: the bytes of
// the bf16 kernel's first trip) behind the first staging round's x requests and ahead of the norm arithmetic, so the HBM stream starts
// at once; the other two go out behind the barrier, when the staging registers are free.  Every wave of the workgroup must call this
// (it holds the barrier).
template <int M, bool NORM, bool STAGE, class F>
__device__ __forceinline__ void w8_prepare(W8X<M, NORM, STAGE>& X, int wave, int lane, float eps, float inv_sqrt_d, F issue) {
    if constexpr (STAGE) {
        uint4 st_x[8], st_s[8];
        const bool stager = wave < M;
        if (stager) gv_stage_load(X.x + (int64_t)wave * X.nvec8, X.scale, X.nvec8, lane, st_x, st_s);
        __builtin_amdgcn_sched_barrier(0);                   // (requests retire in issue order: x ahead of the weights)
        issue();
        if (stager) gv_stage_finish(gv_xn + wave * X.nvec8, X.nvec8, lane, eps, inv_sqrt_d, st_x, st_s);
        if (M > 4) {                                         // batch rows 4-7: a second round for the same waves
            for (int r = wave + 4; r < M; r += 4) {
                gv_stage_load(X.x + (int64_t)r * X.nvec8, X.scale, X.nvec8, lane, st_x, st_s);
                gv_stage_finish(gv_xn + r * X.nvec8, X.nvec8, lane, eps, inv_sqrt_d, st_x, st_s);
            }
        }
        GV_WG_BARRIER();
    } else {
        issue();
        if constexpr (NORM) {
#pragma unroll
            for (int m = 0; m < M; ++m) {
                float ss = 0.f;
                for (int v = lane; v < X.nvec8; v += 64) ss = gv_sumsq8(X.x[(int64_t)m * X.nvec8 + v], ss);
                ss = wave_sum(ss);
                X.inv[m] = 1.0f / (sqrtf(ss) * inv_sqrt_d + eps);
            }
        }
    }
}
// the norm-folding kernels' stream: STAGE -> four slices, the first two requested by w8_prepare's issue(); otherwise the generic loop
template <int M, int R, bool NORM, bool STAGE>
struct W8Rows {
    const uint4* wrow[R];
    uint4 wq[STAGE ? 4 : 1][R];
    template <int I0>
    __device__ __forceinline__ void request(int lane) {
#pragma unroll
        for (int i = I0; i < I0 + 2; ++i)
#pragma unroll
            for (int r = 0; r < R; ++r) wq[i][r] = ld_stream(wrow[r] + lane + 64 * i);
    }
    __device__ __forceinline__ void issue(int lane) {
        if constexpr (STAGE) request<0>(lane);
    }
    __device__ __forceinline__ void run(const W8X<M, NORM, STAGE>& X, int nv, int lane, float (&acc)[R][M]) {
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int m = 0; m < M; ++m) acc[r][m] = 0.f;
        if constexpr (STAGE) {                               // (STAGE launches have nv == 256: the host checks)
            request<2>(lane);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                w8_slice<M, R, (M <= 3)>(wq[i], lane + 64 * i, X, acc);
                if (i == 1) __builtin_amdgcn_sched_barrier(0);   // (trips stay in program order: requests retire in issue order)
            }
        } else {
            w8_stream<M, R, (M <= 3)>(wrow, nv, lane, 64, X, acc);
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int m = 0; m < M; ++m) acc[r][m] = wave_sum(acc[r][m]);
    }
};

// Waves per SIMD each form is compiled for: its bf16 sibling's, as the compiler reports it for csrc/gemv.hip (tests/test_w8_host.py
// reads both code objects and holds these kernels to no scratch and no lower occupancy).  A 16-weight slice meets twice the x a bf16
// slice meets, and left alone the scheduler spends the difference in registers.
constexpr int w8_gemv_waves(int M, bool SPLIT) { return M == 1 ? 8 : M == 2 ? (SPLIT ? 7 : 5) : M == 3 ? 5 : M <= 7 ? 4 : 3; }
constexpr int W8_STAGE_WAVES = 4;

// ---- gemv_kernel on FP8 weights: y = x W^T (+ bias) (+ residual).  SPLIT: the four waves share R rows and each takes every fourth slice.
template <int M, int R, bool SPLIT>
__global__ __launch_bounds__(256, w8_gemv_waves(M, SPLIT)) void w8_gemv_kernel(const uint4* __restrict__ x, const uint4* __restrict__ w, const float* __restrict__ wscale,
                                                      const uint16_t* __restrict__ bias, const uint16_t* res, uint16_t* y, int N,
                                                      int nv) {   // res may alias y; nv = K / 16
    __shared__ float part[SPLIT ? 4 * R * M : 1];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t n0 = SPLIT ? (int64_t)blockIdx.x * R : ((int64_t)blockIdx.x * 4 + wave) * R;
    if (n0 >= N) return;                                     // (workgroup-uniform when SPLIT)
    const uint4* wrow[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t n = n0 + r < N ? n0 + r : N - 1;       // rows past the end are computed on a clamp, not stored
        wrow[r] = w + n * nv;
    }
    // The epilogue is spread over the wave's first R M lanes, one output element (row r, batch row m) each -- the bf16 kernel's lane 0
    // holds R (M + 1) prefetched values, registers this stream needs for x.  Each requests its scale / bias / residual now, not behind
    // the reduction (see gemv_kernel: a dependent ~1 us tail on launches of 5-17 us).
    const int ep_r = lane / M, ep_m = lane - ep_r * M;
    const bool ep_lane = lane < R * M && n0 + ep_r < N && (!SPLIT || wave == 0);
    const int64_t ep_n = ep_lane ? n0 + ep_r : 0;
    float pf_s = 0.f;
    uint16_t pf_b = 0, pf_r = 0;
    if (ep_lane) {
        pf_s = wscale[ep_n];
        if (bias) pf_b = bias[ep_n];
        if (res) pf_r = res[(int64_t)ep_m * N + ep_n];
    }
    float acc[R][M];
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int m = 0; m < M; ++m) acc[r][m] = 0.f;
    const int nvec8 = 2 * nv;
    const auto xf = [&](int m, int j) { return x[(int64_t)m * nvec8 + j]; };
    // (HOLD_X where 8 M < 8 R; the unsplit form keeps it for one row only: at two rows the allocator spilled three registers with it)
    w8_stream<M, R, (M <= (SPLIT ? 3 : 1))>(wrow, nv, SPLIT ? wave * 64 + lane : lane, SPLIT ? 256 : 64, xf, acc);
    float sum = 0.f;                                         // (after wave_sum every lane holds every total: this lane's element)
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const float t = wave_sum(acc[r][m]);
            sum = (ep_r == r && ep_m == m) ? t : sum;
        }
    if (SPLIT) {
        if (lane < R * M) part[wave * R * M + lane] = sum;
        __syncthreads();
        if (wave != 0) return;
        if (lane < R * M) sum = part[lane] + part[R * M + lane] + part[2 * R * M + lane] + part[3 * R * M + lane];
    }
    if (ep_lane) {
        float o = sum * pf_s + (bias ? bf_to_f(pf_b) : 0.f);
        if (res) o += bf_to_f(pf_r);
        y[(int64_t)ep_m * N + ep_n] = f_to_bf(o);
    }
}

// ---- gemv_norm_kernel on FP8 weights: y = bf16(scale * x / (rms(x) + eps)) . W^T + bias
template <int M, int R, bool STAGE>
__global__ __launch_bounds__(256, STAGE ? W8_STAGE_WAVES : 1) void w8_gemv_norm_kernel(const uint4* __restrict__ x, const uint4* __restrict__ scale,
                                                           const uint4* __restrict__ w, const float* __restrict__ wscale,
                                                           const uint16_t* __restrict__ bias, uint16_t* __restrict__ y, int N, int nv,
                                                           float eps, float inv_sqrt_d) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t n0 = ((int64_t)blockIdx.x * 4 + wave) * R;
    if (!STAGE && n0 >= N) return;                           // (STAGE: every wave helps to stage x, then leaves)
    W8Rows<M, R, true, STAGE> W;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const int64_t n = n0 + r < N ? n0 + r : N - 1;
        W.wrow[r] = w + n * nv;
    }
    W8X<M, true, STAGE> X{x, scale, 2 * nv, {}};
    w8_prepare(X, wave, lane, eps, inv_sqrt_d, [&] { W.issue(lane); });
    if (n0 >= N) return;
    float pf_s[R];
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) pf_s[r] = wscale[n0 + r < N ? n0 + r : N - 1];
    }
    float acc[R][M];
    W.run(X, nv, lane, acc);
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t n = n0 + r;
            if (n < N) {
                const float b = bias ? bf_to_f(bias[n]) : 0.f;
#pragma unroll
                for (int m = 0; m < M; ++m) y[(int64_t)m * N + n] = f_to_bf(acc[r][m] * pf_s[r] + b);
            }
        }
    }
}

// ---- gemv_norm_hyena_kernel on FP8 weights: pre-norm + projection + FIR / modal step + gate in one launch.  A wave owns CPW adjacent
// channels of one head = 3 CPW rows of the projection; its first CPW * M lanes run evo_hyena_step's arithmetic on the scaled dot products,
// statement for statement the bf16 kernel's epilogue.
template <int M, int CPW, bool STAGE>
__global__ __launch_bounds__(256) void w8_gemv_norm_hyena_kernel(
    const uint4* __restrict__ x, const uint4* __restrict__ scale, const uint4* __restrict__ w, const float* __restrict__ wscale,
    const uint16_t* __restrict__ bias, uint16_t* __restrict__ fir_state, float* __restrict__ iir_state,
    const uint16_t* __restrict__ fir_w, const uint16_t* __restrict__ fir_b, const float* __restrict__ poles,
    const float* __restrict__ residues, const uint16_t* __restrict__ dskip, uint16_t* __restrict__ y, int D, int nv,
    float eps, float inv_sqrt_d) {
    constexpr int HDc = 128, NSc = 8, R = 3 * CPW;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int unit = blockIdx.x * 4 + wave;                     // channel (pair) index over D / CPW
    if (!STAGE && unit >= D / CPW) return;
    const int unit_c = unit < D / CPW ? unit : D / CPW - 1;     // (STAGE: a wave past the end stages x with the others, then leaves)
    const int h = unit_c / (HDc / CPW), j0 = CPW * (unit_c - h * (HDc / CPW));
    W8Rows<M, R, true, STAGE> W;
#pragma unroll
    for (int r = 0; r < R; ++r) W.wrow[r] = w + (int64_t)(h * 3 * HDc + (r / CPW) * HDc + j0 + (r % CPW)) * nv;
    W8X<M, true, STAGE> X{x, scale, 2 * nv, {}};
    w8_prepare(X, wave, lane, eps, inv_sqrt_d, [&] { W.issue(lane); });
    if (unit >= D / CPW) return;
    // the epilogue's operands (this lane's channel x batch row) are requested now, behind the weights: they do not depend on the sums
    const bool ep_lane = lane < CPW * M;
    const int ep_e = lane % CPW, ep_m = ep_lane ? lane / CPW : 0;
    const int ep_dch = h * HDc + j0 + ep_e;
    float pf_ws[3];
    uint16_t pf_bias[3], pf_fw[3][3], pf_fb[3], pf_fs[3][2], pf_dk = 0;
    float2 pf_p[NSc], pf_r[NSc], pf_s[NSc];
    if (ep_lane) {
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            const int c = h * 3 * HDc + g * HDc + j0 + ep_e;
            pf_ws[g] = wscale[c];
            pf_bias[g] = bias[c];
            pf_fw[g][0] = fir_w[c * 3]; pf_fw[g][1] = fir_w[c * 3 + 1]; pf_fw[g][2] = fir_w[c * 3 + 2];
            pf_fb[g] = fir_b[c];
            const uint16_t* fs = fir_state + ((int64_t)ep_m * 3 * D + c) * 2;
            pf_fs[g][0] = fs[0]; pf_fs[g][1] = fs[1];
        }
        const float2* st = (const float2*)iir_state + ((int64_t)ep_m * D + ep_dch) * NSc;
        const float2* pp = (const float2*)poles + (int64_t)ep_dch * NSc;
        const float2* rp = (const float2*)residues + (int64_t)ep_dch * NSc;
#pragma unroll
        for (int sI = 0; sI < NSc; ++sI) { pf_p[sI] = pp[sI]; pf_r[sI] = rp[sI]; pf_s[sI] = st[sI]; }
        pf_dk = dskip[ep_dch];
    }
    float acc[R][M];
    W.run(X, nv, lane, acc);
    if (!ep_lane) return;
    const int e = ep_e, m = ep_m;                                // this lane: channel j0 + e of batch row m
    float f[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {
        float d = 0.f;
#pragma unroll
        for (int mm = 0; mm < M; ++mm)
#pragma unroll
            for (int ee = 0; ee < CPW; ++ee) d = (m == mm && e == ee) ? acc[CPW * g + ee][mm] : d;
        const int c = h * 3 * HDc + g * HDc + j0 + e;            // channel in the 3D row
        const uint16_t zraw = f_to_bf(d * pf_ws[g] + bf_to_f(pf_bias[g]));   // what the unfused projection stores
        uint16_t* fs = fir_state + ((int64_t)m * 3 * D + c) * 2;
        const float o0 = bf_to_f(pf_fs[g][0]), o1 = bf_to_f(pf_fs[g][1]);
        f[g] = fmaf(bf_to_f(pf_fw[g][2]), bf_to_f(zraw),
                    fmaf(bf_to_f(pf_fw[g][1]), o1, fmaf(bf_to_f(pf_fw[g][0]), o0, bf_to_f(pf_fb[g]))));
        fs[0] = pf_fs[g][1];
        fs[1] = zraw;
    }
    const float xv = f[1] * f[2];
    float2* st = (float2*)iir_state + ((int64_t)m * D + ep_dch) * NSc;
    float accy = 0.f;
#pragma unroll
    for (int s = 0; s < NSc; ++s) {
        const float2 p = pf_p[s], r = pf_r[s], sv = pf_s[s];
        const float nr = fmaf(p.x, sv.x, fmaf(-p.y, sv.y, xv));
        const float ni = fmaf(p.x, sv.y, p.y * sv.x);
        st[s] = make_float2(nr, ni);
        accy = fmaf(r.x, nr, fmaf(-r.y, ni, accy));
    }
    y[(int64_t)m * D + ep_dch] = f_to_bf(fmaf(xv, bf_to_f(pf_dk), accy) * f[0]);
}

// ---- gemv_gate_kernel on FP8 weights: a[m][n] = gelu(x_m . W1_n) * (x_m . W2_n), W12 = [W1; W2] plain or grouped; NORM: x is the raw
// residual row.  A wave owns 2 output columns = rows (n, n + 1) of W1 and of W2; both (scaled) sums are rounded to bf16, then the gate.
template <int M, bool NORM, bool STAGE>
__global__ __launch_bounds__(256, STAGE ? W8_STAGE_WAVES : 1) void w8_gemv_gate_kernel(const uint4* __restrict__ x, const uint4* __restrict__ scale,
                                                           const uint4* __restrict__ w, const float* __restrict__ wscale,
                                                           uint16_t* __restrict__ a, int I, int nv, float eps, float inv_sqrt_d,
                                                           int grouped) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int64_t n0 = ((int64_t)blockIdx.x * 4 + wave) * 2;
    if (!STAGE && n0 >= I) return;
    W8Rows<M, 4, NORM, STAGE> W;
    int64_t rows[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t n = n0 + (r & 1) < I ? n0 + (r & 1) : I - 1;
        // plain [W1; W2]: row (r >> 1) I + n.  grouped (pack_gate_weights): row 64 (n / 32) + 32 (r >> 1) + n % 32
        rows[r] = grouped ? 64 * (n >> 5) + 32 * (r >> 1) + (n & 31) : (r >> 1) * (int64_t)I + n;
        W.wrow[r] = w + rows[r] * nv;
    }
    W8X<M, NORM, STAGE> X{x, scale, 2 * nv, {}};
    w8_prepare(X, wave, lane, eps, inv_sqrt_d, [&] { W.issue(lane); });
    if (n0 >= I) return;
    float pf_s[4];
    if (lane == 0) {
#pragma unroll
        for (int r = 0; r < 4; ++r) pf_s[r] = wscale[rows[r]];
    }
    float acc[4][M];
    W.run(X, nv, lane, acc);
    if (lane == 0) {
#pragma unroll
        for (int m = 0; m < M; ++m) {
            const f32x2_t u = {round_bf(acc[0][m] * pf_s[0]), round_bf(acc[1][m] * pf_s[1])};
            const f32x2_t g = {round_bf(acc[2][m] * pf_s[2]), round_bf(acc[3][m] * pf_s[3])};
            const f32x2_t o = gelu_gate2(u, g);
            if (n0 + 1 < I) *(uint32_t*)(a + (int64_t)m * I + n0) = pack_bf2(o[0], o[1]);
            else a[(int64_t)m * I + n0] = f_to_bf(o[0]);
        }
    }
}

// ---- host side ---------------------------------------------------------------------------------------------------------------------
static bool w8_aligned(const void* p, uintptr_t a) { return p && ((uintptr_t)p & (a - 1)) == 0; }
static bool w8_aligned_or_null(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }
// x / weight / scale / output of every compute entry, and the shape rules they share
static bool w8_common_ok(const void* x, const void* w_data, const float* w_scale, const void* y, int64_t M, int64_t N, int64_t K) {
    return w8_aligned(x, 16) && w8_aligned(w_data, 16) && w8_aligned(w_scale, 4) && w8_aligned(y, 16) && M >= 1 && M <= 8 && N > 0 &&
           K > 0 && K % 16 == 0 && N <= 0x7fffffff - 16;
}

extern "C" int evo_w_quant_fp8(const void* w, void* w_data, float* w_scale, int64_t N, int64_t K, void* stream) {
    if (!w8_aligned(w, 16) || !w8_aligned(w_data, 16) || !w8_aligned(w_scale, 4) || N <= 0 || K <= 0 || K % 16 != 0 || N > 0x7fffffff)
        return -1;
    hipLaunchKernelGGL(w_quant_fp8_kernel, dim3((unsigned)N), dim3(256), 0, (hipStream_t)stream, (const uint4*)w, (uint2*)w_data, w_scale,
                       (int)(K / 8));
    return evo_launch_status();
}

extern "C" int evo_linear_small_m_w8(const void* x, const void* w_data, const float* w_scale, const void* bias, const void* residual,
                                     void* y, int64_t M, int64_t N, int64_t K, void* ws, int64_t ws_bytes, void* stream) {
    (void)ws; (void)ws_bytes;                                // (the bf16 entry's workspace serves its 17-64-row forms: none here)
    if (!w8_common_ok(x, w_data, w_scale, y, M, N, K) || !w8_aligned_or_null(bias, 16) || !w8_aligned_or_null(residual, 16)) return -1;
    constexpr int R = 4;                                     // rows per wave and the SPLIT rule: gemv_launch's (csrc/gemv.hip)
    const int64_t waves = (N + R - 1) / R;
    for_m(M, [&](auto m) {
        const auto launch = [&](auto split, int64_t groups) {
            hipLaunchKernelGGL((w8_gemv_kernel<decltype(m)::value, R, decltype(split)::value>), dim3((unsigned)groups), dim3(256), 0,
                               (hipStream_t)stream, (const uint4*)x, (const uint4*)w_data, w_scale, (const uint16_t*)bias,
                               (const uint16_t*)residual, (uint16_t*)y, (int)N, (int)(K / 16));
        };
        if (N <= 4096 && K >= 2048) launch(std::true_type{}, waves); else launch(std::false_type{}, (waves + 3) / 4);
    });
    return evo_launch_status();
}

extern "C" int evo_norm_linear_small_m_w8(const void* x, const void* scale, const void* w_data, const float* w_scale, const void* bias,
                                          void* y, int64_t M, int64_t N, int64_t K, float eps, void* stream) {
    if (!w8_common_ok(x, w_data, w_scale, y, M, N, K) || !w8_aligned(scale, 16) || !w8_aligned_or_null(bias, 16)) return -1;
    if (M > 4 && K != 4096) return -1;                       // batches of 5-8 rows exist in the LDS-staged form only
    const dim3 grid((unsigned)(((N + 3) / 4 + 3) / 4)), block(256);
    const float isd = 1.0f / sqrtf((float)K);
    for_m_stage(M, K == 4096, [&](auto m, auto st) {
        constexpr bool ST = decltype(st)::value;
        hipLaunchKernelGGL((w8_gemv_norm_kernel<decltype(m)::value, 4, ST>), grid, block, ST ? (size_t)M * K * 2 : 0, (hipStream_t)stream,
                           (const uint4*)x, (const uint4*)scale, (const uint4*)w_data, w_scale, (const uint16_t*)bias, (uint16_t*)y, (int)N,
                           (int)(K / 16), eps, isd);
    });
    return evo_launch_status();
}

extern "C" int evo_hyena_decode_fused_small_m_w8(const void* x, const void* norm_scale, const void* proj_data, const float* proj_scale,
                                                 const void* proj_b, void* fir_state, float* iir_state, const void* fir_w,
                                                 const void* fir_b, const float* poles, const float* residues, const void* dskip,
                                                 void* y, int64_t M, int64_t D, int64_t n_heads, float eps, void* stream) {
    if (!w8_common_ok(x, proj_data, proj_scale, y, M, 3 * D, D) || D != n_heads * 128) return -1;
    if (!w8_aligned(norm_scale, 16) || !w8_aligned(proj_b, 16) || !w8_aligned(fir_state, 16) || !w8_aligned(iir_state, 16) ||
        !w8_aligned(fir_w, 16) || !w8_aligned(fir_b, 16) || !w8_aligned(poles, 16) || !w8_aligned(residues, 16) || !w8_aligned(dskip, 16))
        return -1;
    if (M > 4 && D != 4096) return -1;                       // batches of 5-8 rows exist in the LDS-staged form only
    const float isd = 1.0f / sqrtf((float)D);
    for_m_stage(M, D == 4096, [&](auto m, auto st) {
        constexpr int MM = decltype(m)::value;
        constexpr bool ST = decltype(st)::value;
        constexpr int CPW = !ST && (MM == 2 || MM == 3) ? 2 : 1;     // channels per wave: the bf16 entry's choice
        hipLaunchKernelGGL((w8_gemv_norm_hyena_kernel<MM, CPW, ST>), dim3((unsigned)((D / CPW + 3) / 4)), dim3(256), ST ? (size_t)M * D * 2 : 0,
                           (hipStream_t)stream, (const uint4*)x, (const uint4*)norm_scale, (const uint4*)proj_data, proj_scale,
                           (const uint16_t*)proj_b, (uint16_t*)fir_state, iir_state, (const uint16_t*)fir_w, (const uint16_t*)fir_b, poles,
                           residues, (const uint16_t*)dskip, (uint16_t*)y, (int)D, (int)(D / 16), eps, isd);
    });
    return evo_launch_status();
}

static int w8_gate_launch(const void* x, const void* scale, const void* w12_data, const float* w12_scale, void* a, int64_t M, int64_t I,
                          int64_t K, float eps, int64_t grouped, hipStream_t s) {
    if (!w8_common_ok(x, w12_data, w12_scale, a, M, I, K) || I % 2 != 0 || I > 0x3fffffff || (grouped && I % 32 != 0)) return -1;
    if (scale && M > 4 && K != 4096) return -1;              // with the norm, batches of 5-8 rows exist in the LDS-staged form only
    const dim3 grid((unsigned)((I / 2 + 3) / 4)), block(256);
    const float isd = 1.0f / sqrtf((float)K);
    const int grp = grouped ? 1 : 0;
    const auto launch = [&](auto m, auto norm, auto st) {
        constexpr bool NORM = decltype(norm)::value, ST = decltype(st)::value;
        hipLaunchKernelGGL((w8_gemv_gate_kernel<decltype(m)::value, NORM, ST>), grid, block, ST ? (size_t)M * K * 2 : 0, s, (const uint4*)x,
                           (const uint4*)scale, (const uint4*)w12_data, w12_scale, (uint16_t*)a, (int)I, (int)(K / 16), NORM ? eps : 0.f,
                           NORM ? isd : 0.f, grp);
    };
    if (scale) for_m_stage(M, K == 4096, [&](auto m, auto st) { launch(m, std::true_type{}, st); });
    else for_m(M, [&](auto m) { launch(m, std::false_type{}, std::false_type{}); });
    return evo_launch_status();
}

extern "C" int evo_mlp_gate_small_m_w8(const void* x, const void* w12_data, const float* w12_scale, void* a, int64_t M, int64_t I,
                                       int64_t K, int64_t grouped, void* stream) {
    return w8_gate_launch(x, nullptr, w12_data, w12_scale, a, M, I, K, 0.f, grouped, (hipStream_t)stream);
}

extern "C" int evo_norm_mlp_gate_small_m_w8(const void* x, const void* scale, const void* w12_data, const float* w12_scale, void* a,
                                            int64_t M, int64_t I, int64_t K, float eps, int64_t grouped, void* stream) {
    if (!w8_aligned(scale, 16)) return -1;
    return w8_gate_launch(x, scale, w12_data, w12_scale, a, M, I, K, eps, grouped, (hipStream_t)stream);
}
