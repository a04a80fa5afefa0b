// Per-row Hyena end state of a RAGGED batch, from channel-major z^T (gfx950).
//
// A cached prefill hands decode the modal state and the two steps of FIR history at the row's LAST token.  evo_hyena_ct and
// evo_hyena_carry_scan know one T for the whole batch; a batch of right-padded prompts of unequal length needs the state at
// lens[b] - 1 of every row b, and the state at T cannot be rolled back (that would divide by p^(T - L), |p| < 1).  This file
// computes it directly, reading only the x1 | v thirds of z^T, positions t < lens[b]:
//   launch 1  partial : a thread owns (row b, segment k of HR_SEG steps, channel d) and walks the segment from a zero state --
//                       the per-step arithmetic of hyena_seg_state_kernel (csrc/hyena.hip): FIR in fp32, x = x1 * v in fp32, the
//                       eight modes S <- p S + x in fp32.  Its eight consecutive steps of a signal are 16 contiguous bytes of z^T
//                       (one global_load_dwordx4, as in csrc/hyena_ct.hip).  Segments wholly behind lens[b] exit at once; the
//                       segment that holds lens[b] - 1 stops there.
//   launch 2  combine : a thread owns (b, d, mode): Horner over the row's segments with p^HR_SEG in fp64 (cpow_int, as
//                       hyena_carry_scan_kernel does), the ragged last segment with p^(steps it holds); threads of modes 0..2
//                       also copy the two history steps of the x2 / x1 / v column of their channel, bits untouched.
// Both launches have grids fixed by (B, T, D): lens is read on the device only.  Nothing at t >= lens[b] reaches an output: such
// steps may be LOADED (the 16 bytes that hold step lens[b] - 1 hold up to seven steps behind it) but never enter arithmetic.
// Cost (profiles/prefill_batch_notes.txt): 85 us at 8 x 1,024 x 4,096 where the operator's launch takes 64 -- the
// lanes of launch 1 are adjacent CHANNELS, 512 bytes apart in z^T, so a load instruction touches 64 cache lines; lanes along time with
// a transposition in front of the recurrence is the open item.
// Entry point and reference citation: include/evo_mi355x.h (evo_hyena_state_at_zt).
#include "common.h"
#include "../../include/evo_mi355x.h"

#define HR_NS 8                 // state_size
#define HR_HD 128               // channels per head = threads per workgroup of launch 1
#define HR_SEG EVO_HYENA_RAGGED_SEG
#define HR_ZBLK 256             // positions per block of z^T
static_assert(HR_SEG % 8 == 0, "a segment is a whole number of 16-byte loads");

typedef uint32_t hr_u32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ int64_t hr_len(const int64_t* __restrict__ lens, int b, int64_t T) {
    int64_t n = lens[b];
    n = n < 1 ? 1 : n;
    return n > T ? T : n;
}

// byte offset of position p inside a column of z^T (behind the column's base c * 512)
__device__ __forceinline__ int64_t hr_off(int64_t p, int64_t blk_bytes) { return (p / HR_ZBLK) * blk_bytes + (p % HR_ZBLK) * 2; }

__device__ __forceinline__ void hr_cpow(double pr, double pi, int64_t n, double& or_, double& oi) {
    double rr = 1.0, ri = 0.0;
    while (n > 0) {
        if (n & 1) { double t = rr * pr - ri * pi; ri = rr * pi + ri * pr; rr = t; }
        double t = pr * pr - pi * pi; pi = 2.0 * pr * pi; pr = t;
        n >>= 1;
    }
    or_ = rr; oi = ri;
}

// ------------------------------------------------------------------------------------------------ launch 1
__global__ __launch_bounds__(HR_HD) void hyena_ragged_partial_kernel(
    const unsigned char* __restrict__ zt, const int64_t* __restrict__ lens, const uint16_t* __restrict__ fir_w,
    const uint16_t* __restrict__ fir_b, const float2* __restrict__ poles, float4* __restrict__ part, int64_t T, int D, int H,
    int n_seg, int64_t row_pitch, int64_t zt_row0) {
    const int64_t blk = blockIdx.x;                                    // over B * n_seg * H, head fastest
    const int h = (int)(blk % H);
    const int seg = (int)((blk / H) % n_seg);
    const int b = (int)(blk / ((int64_t)H * n_seg));
    const int64_t len = hr_len(lens, b, T);
    const int64_t t0 = (int64_t)seg * HR_SEG;
    if (t0 >= len) return;                                             // wholly behind the row's last token
    const int64_t t1 = t0 + HR_SEG < len ? t0 + HR_SEG : len;
    const int j = threadIdx.x;
    const int d = h * HR_HD + j;
    const int c1 = h * 3 * HR_HD + HR_HD + j, c2 = c1 + HR_HD;         // x1 and v columns of the channel [REF model.py: x2 | x1 | v per head]
    const int64_t blk_bytes = (int64_t)D * 3 * (HR_ZBLK * 2);
    const unsigned char* z1 = zt + (int64_t)c1 * (HR_ZBLK * 2);
    const unsigned char* z2 = zt + (int64_t)c2 * (HR_ZBLK * 2);
    const int64_t p0 = zt_row0 + (int64_t)b * row_pitch;               // position of the row's step 0 (% 8 == 0)

    float w1[3], w2[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { w1[k] = bf_to_f(fir_w[c1 * 3 + k]); w2[k] = bf_to_f(fir_w[c2 * 3 + k]); }
    const float b1 = bf_to_f(fir_b[c1]), b2 = bf_to_f(fir_b[c2]);
    float pr[HR_NS], pi[HR_NS], sr[HR_NS], si[HR_NS];
#pragma unroll
    for (int s = 0; s < HR_NS; ++s) {
        const float2 p = poles[(int64_t)d * HR_NS + s];
        pr[s] = p.x; pi[s] = p.y; sr[s] = 0.f; si[s] = 0.f;
    }
    // steps t0 - 2, t0 - 1: one dword of the previous 16-byte group (same block of z^T: (p0 + t0) % 8 == 0); zeros before t = 0
    float m2a = 0.f, m1a = 0.f, m2b = 0.f, m1b = 0.f;
    if (t0 > 0) {
        const int64_t o = hr_off(p0 + t0 - 2, blk_bytes);
        const uint32_t ha = *(const uint32_t*)(z1 + o), hb = *(const uint32_t*)(z2 + o);
        m2a = bf_lo(ha); m1a = bf_hi(ha); m2b = bf_lo(hb); m1b = bf_hi(hb);
    }
    auto step = [&](float ca, float cb) {
        const float x1c = fmaf(w1[2], ca, fmaf(w1[1], m1a, fmaf(w1[0], m2a, b1)));
        const float vc = fmaf(w2[2], cb, fmaf(w2[1], m1b, fmaf(w2[0], m2b, b2)));
        const float x = x1c * vc;
        float tt[HR_NS], uu[HR_NS];
#pragma unroll
        for (int s = 0; s < HR_NS; ++s) tt[s] = fmaf(-pi[s], si[s], x);
#pragma unroll
        for (int s = 0; s < HR_NS; ++s) uu[s] = pi[s] * sr[s];
#pragma unroll
        for (int s = 0; s < HR_NS; ++s) sr[s] = fmaf(pr[s], sr[s], tt[s]);
#pragma unroll
        for (int s = 0; s < HR_NS; ++s) si[s] = fmaf(pr[s], si[s], uu[s]);
        m2a = m1a; m1a = ca; m2b = m1b; m1b = cb;
    };
    // eight steps per iteration; the next group's loads are issued before this group's arithmetic
    int64_t o = hr_off(p0 + t0, blk_bytes);
    hr_u32x4 ra = *(const hr_u32x4*)(z1 + o), rb = *(const hr_u32x4*)(z2 + o);
    for (int64_t t = t0; t < t1; t += 8) {
        const hr_u32x4 ca = ra, cb = rb;
        if (t + 8 < t1) {                                              // (block-uniform: one row, one segment per workgroup)
            o = hr_off(p0 + t + 8, blk_bytes);
            ra = *(const hr_u32x4*)(z1 + o);
            rb = *(const hr_u32x4*)(z2 + o);
        }
        if (t + 8 <= t1) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                step(bf_lo(ca[i]), bf_lo(cb[i]));
                step(bf_hi(ca[i]), bf_hi(cb[i]));
            }
        } else {                                                       // the group that holds the row's last token
            const int n = (int)(t1 - t);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (2 * i < n) step(bf_lo(ca[i]), bf_lo(cb[i]));
                if (2 * i + 1 < n) step(bf_hi(ca[i]), bf_hi(cb[i]));
            }
        }
    }
    float4* out = part + ((((int64_t)b * n_seg + seg) * D + d) * HR_NS) / 2;
#pragma unroll
    for (int s = 0; s < HR_NS; s += 2) out[s / 2] = make_float4(sr[s], si[s], sr[s + 1], si[s + 1]);
}

// ------------------------------------------------------------------------------------------------ launch 2
__global__ __launch_bounds__(256) void hyena_ragged_combine_kernel(
    const unsigned char* __restrict__ zt, const int64_t* __restrict__ lens, const float2* __restrict__ poles,
    const float2* __restrict__ part, float2* __restrict__ s_out, uint32_t* __restrict__ fir_out, int B, int64_t T, int D,
    int n_seg, int64_t row_pitch, int64_t zt_row0) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;        // over B * D * 8
    const int64_t per_b = (int64_t)D * HR_NS;
    if (i >= (int64_t)B * per_b) return;
    const int b = (int)(i / per_b);
    const int64_t ds = i - (int64_t)b * per_b;
    const int64_t len = hr_len(lens, b, T);
    const float2 p = poles[ds];
    double pcr, pci;
    hr_cpow((double)p.x, (double)p.y, HR_SEG, pcr, pci);
    const int n_lead = (int)((len - 1) / HR_SEG);                      // whole segments in front of the one that holds the last token
    const float2* a = part + (int64_t)b * n_seg * per_b + ds;
    double rr = 0.0, ri = 0.0;
    for (int k = 0; k < n_lead; ++k) {
        const float2 v = a[(int64_t)k * per_b];
        const double nr = pcr * rr - pci * ri + (double)v.x;
        ri = pcr * ri + pci * rr + (double)v.y;
        rr = nr;
    }
    {
        const float2 v = a[(int64_t)n_lead * per_b];
        double qr, qi;
        hr_cpow((double)p.x, (double)p.y, len - (int64_t)n_lead * HR_SEG, qr, qi);
        const double nr = qr * rr - qi * ri + (double)v.x;
        ri = qr * ri + qi * rr + (double)v.y;
        rr = nr;
    }
    s_out[i] = make_float2((float)rr, (float)ri);

    // FIR history: steps len - 2, len - 1 of column (signal g = mode index, channel d), oldest first, zeros before t = 0
    const int g = (int)(ds % HR_NS);
    if (g < 3) {
        const int d = (int)(ds / HR_NS);
        const int c = (d / HR_HD) * 3 * HR_HD + g * HR_HD + d % HR_HD;
        const int64_t blk_bytes = (int64_t)D * 3 * (HR_ZBLK * 2);
        const unsigned char* zc = zt + (int64_t)c * (HR_ZBLK * 2);
        const int64_t p0 = zt_row0 + (int64_t)b * row_pitch;
        const uint32_t last = *(const uint16_t*)(zc + hr_off(p0 + len - 1, blk_bytes));
        const uint32_t prev = len >= 2 ? *(const uint16_t*)(zc + hr_off(p0 + len - 2, blk_bytes)) : 0u;
        fir_out[(int64_t)b * 3 * D + c] = prev | (last << 16);
    }
}

// ------------------------------------------------------------------------------------------------ C ABI
extern "C" int evo_hyena_state_at_zt(const void* zt, const int64_t* lens, const void* fir_w, const void* fir_b, const float* poles,
                                     float* s_out, void* fir_out, float* ws, int64_t ws_bytes, int64_t B, int64_t T, int64_t D,
                                     int64_t n_heads, int64_t zt_pitch, int64_t row_pitch, int64_t zt_row0, void* stream) {
    if (B <= 0 || T <= 0 || D <= 0 || n_heads <= 0 || D != n_heads * HR_HD) return -1;
    if (T % 64 != 0 && B != 1) return -1;                              // the plain form of the z^T layout
    if (row_pitch % 8 != 0 || (B > 1 && row_pitch < T) || row_pitch < 0) return -1;
    if (zt_row0 < 0 || zt_row0 % 8 != 0 || zt_pitch % HR_ZBLK != 0 || zt_pitch < HR_ZBLK) return -1;
    if (zt_row0 + (B - 1) * row_pitch + T > zt_pitch) return -1;
    if (!zt || !lens || !fir_w || !fir_b || !poles || !s_out || !fir_out) return -1;
    if (((uintptr_t)zt & 15) != 0) return -1;
    const int64_t n_seg = (T + HR_SEG - 1) / HR_SEG;
    const int64_t blocks = B * n_seg * n_heads;
    const int64_t need = B * n_seg * D * HR_NS * 8;
    if (need > 0x7fffffffll || blocks > 0x7fffffffll || B * D * HR_NS / 256 + 1 > 0x7fffffffll) return -1;
    if (!ws) return (int)need;                                         // the workspace query
    if (ws_bytes < need || ((uintptr_t)ws & 15) != 0) return -1;
    hipLaunchKernelGGL(hyena_ragged_partial_kernel, dim3((unsigned)blocks), dim3(HR_HD), 0, (hipStream_t)stream,
                       (const unsigned char*)zt, lens, (const uint16_t*)fir_w, (const uint16_t*)fir_b, (const float2*)poles,
                       (float4*)ws, T, (int)D, (int)n_heads, (int)n_seg, row_pitch, zt_row0);
    const int64_t n = B * D * HR_NS;
    hipLaunchKernelGGL(hyena_ragged_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const unsigned char*)zt, lens, (const float2*)poles, (const float2*)ws, (float2*)s_out,
                       (uint32_t*)fir_out, (int)B, T, (int)D, (int)n_seg, row_pitch, zt_row0);
    return evo_launch_status();
}
