// FP8 (OCP e4m3fn) KV cache for decode: the quantising stores and the decode attention that reads them (include/evo_mi355x.h, ABI 19).
//
// THE RULE (the host reference in tests/test_kv_fp8_host.py states it in torch; both sides agree bit for bit).  A cached row is the 128
// values of one (stream, token, K-or-V, head).  With a = max |x_j| over the row, e is the smallest integer with a 2^-e <= 448, clamped to
// [-126, 120] (a = 0: e = 0).  Stored: 128 bytes RNE_e4m3fn(x_j 2^-e) and ONE f32 scale 2^e.  x_j 2^-e is exact in fp32 and at most 448 in
// magnitude, so the conversion rounds once and never saturates; byte * scale is exact in fp32.  e comes from the exponent and mantissa
// bits of a (a bf16 value: 448 = 1.75 * 2^8, so the mantissa decides between two neighbouring exponents), never from a logarithm.
//
// Layout of a layer: data [B, cap, 2, H, 128] bytes (the bf16 cache's layout, byte-wide), scale [B, 2, H, cap] f32 -- token-contiguous per
// head, so that the 64 scales of a key block are one 256-byte run for the wave that streams that head.
#include "common.h"
#include "../../include/evo_mi355x.h"

#include "attn_common.h"
#include "fp8_common.h"            // the rule's device code: fp8_row_exponent, fp8_pow2, fp8_group_max, fp8_quant8

struct KvFp8Cache {                // the cache operand of all three launches
    uint8_t* data; float* scale;
    int64_t d_sb, d_st, d_sw, d_sh;    // bytes: batch, token, k|v, head
    int64_t s_sb, s_sw, s_sh;          // floats: batch, k|v, head (token stride 1)
};

// ---- evo_kv_quant_fp8: rows [B, T, H, 128] of K and of V -> cache tokens t0 .. t0 + T - 1.  A row is 256 bytes = 16 lanes x 16 bytes: a wave
// takes four rows, the row maximum is a 16-lane DPP reduction, one pass, no LDS.  Rows are numbered (b, t, k|v, h) with h fastest: the
// source rows of a token are neighbours in a packed qkv and so are the cache rows written.
__global__ __launch_bounds__(256) void kv_quant_fp8_kernel(const uint16_t* __restrict__ k, const uint16_t* __restrict__ v, KvFp8Cache c,
                                                           int64_t n_rows, int T, int H, int64_t t0, int64_t k_sb, int64_t k_st,
                                                           int64_t k_sh, int64_t v_sb, int64_t v_st, int64_t v_sh) {
    const int64_t r = (int64_t)blockIdx.x * 16 + (threadIdx.x >> 4);
    if (r >= n_rows) return;                                 // whole 16-lane groups leave together
    const int dc = threadIdx.x & 15;
    const int h = (int)(r % H);
    int64_t x = r / H;
    const int which = (int)(x & 1);
    x >>= 1;
    const int64_t t = x % T, b = x / T;
    const uint16_t* src = which ? v + b * v_sb + t * v_st + h * v_sh : k + b * k_sb + t * k_st + h * k_sh;
    const uint4 val = ((const uint4*)src)[dc];
    const int e = fp8_row_exponent(fp8_group_max<16>(fp8_max15(val)));
    uint8_t* drow = c.data + b * c.d_sb + (t0 + t) * c.d_st + which * c.d_sw + h * c.d_sh;
    ((uint2*)drow)[dc] = fp8_quant8(val, fp8_pow2(-e));
    if (dc == 0) c.scale[b * c.s_sb + which * c.s_sw + h * c.s_sh + t0 + t] = fp8_pow2(e);
}

// ---- evo_rope_append_decode_fp8: rope_append_decode_kernel (csrc/elementwise.hip) with the append quantised.  The rotary arithmetic is
// that kernel's, statement for statement, so the q and k left in qkv carry its bits.  hd = 128: the 8 lanes of a (row, head) hold the
// head's 128 values (chunks c and c + 8 each), so the row maximum is an 8-lane DPP reduction.
__device__ __forceinline__ void fp8_unpack8(const uint4& v, float* f) {
    f[0] = bf_lo(v.x); f[1] = bf_hi(v.x); f[2] = bf_lo(v.y); f[3] = bf_hi(v.y);
    f[4] = bf_lo(v.z); f[5] = bf_hi(v.z); f[6] = bf_lo(v.w); f[7] = bf_hi(v.w);
}
__device__ __forceinline__ uint4 fp8_pack8(const float* f) {
    uint4 v;
    v.x = pack_bf2(f[0], f[1]); v.y = pack_bf2(f[2], f[3]); v.z = pack_bf2(f[4], f[5]); v.w = pack_bf2(f[6], f[7]);
    return v;
}
// one head row held as chunks (r0 = chunk c, r1 = chunk c + 8) by 8 lanes -> cache row `drow` and its scale
__device__ __forceinline__ void fp8_store_row8(const uint4& r0, const uint4& r1, uint8_t* drow, float* srow, int c) {
    const int e = fp8_row_exponent(fp8_group_max<8>(max(fp8_max15(r0), fp8_max15(r1))));
    const float inv = fp8_pow2(-e);
    ((uint2*)drow)[c] = fp8_quant8(r0, inv);
    ((uint2*)drow)[8 + c] = fp8_quant8(r1, inv);
    if (c == 0) *srow = fp8_pow2(e);
}

__global__ __launch_bounds__(256) void rope_append_decode_fp8_kernel(uint4* __restrict__ qkv, KvFp8Cache kc,
                                                                     const int64_t* __restrict__ pos,
                                                                     const float* __restrict__ inv_freq, float scaling, int B,
                                                                     int H, float q_scale) {
    const int hd = 128;
    const int half_vec = hd / 16;
    const int total = B * H * half_vec;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;                                  // whole 8-lane groups leave together
    const int c = i % half_vec;
    const int h = (i / half_vec) % H;
    const int b = i / (half_vec * H);
    const int64_t p = pos[b];
    float t = (float)p;
    if (scaling != 1.0f) t = t / scaling;
    float co[8], si[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float f = t * inv_freq[c * 8 + e];
        co[e] = round_bf(cosf(f));
        si[e] = round_bf(sinf(f));
    }
    const int rv = hd / 8;                                   // vectors per head row
    uint4 k0, k1;
#pragma unroll
    for (int which = 0; which < 2; ++which) {                // q, k
        const int64_t row_vec = (((int64_t)b * 3 + which) * H + h) * rv;
        float x0[8], x1[8], o0[8], o1[8];
        fp8_unpack8(qkv[row_vec + c], x0);
        fp8_unpack8(qkv[row_vec + half_vec + c], x1);
        const float qs = which == 0 ? q_scale : 1.0f;         // (see rope_kernel)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            o0[e] = (x0[e] * co[e] - x1[e] * si[e]) * qs;
            o1[e] = (x0[e] * si[e] + x1[e] * co[e]) * qs;
        }
        const uint4 r0 = fp8_pack8(o0), r1 = fp8_pack8(o1);
        qkv[row_vec + c] = r0;
        qkv[row_vec + half_vec + c] = r1;
        if (which == 1) { k0 = r0; k1 = r1; }
    }
    uint8_t* drow = kc.data + b * kc.d_sb + p * kc.d_st + h * kc.d_sh;
    float* srow = kc.scale + b * kc.s_sb + h * kc.s_sh + p;
    fp8_store_row8(k0, k1, drow, srow, c);
    const int64_t vvec = (((int64_t)b * 3 + 2) * H + h) * rv;
    fp8_store_row8(qkv[vvec + c], qkv[vvec + half_vec + c], drow + kc.d_sw, srow + kc.s_sw, c);
}

// ---- evo_attn_decode_fp8: attn_decode_stream_kernel (csrc/attn.hip) on the FP8 cache -- a wave owns a split (blocks s, s + n_splits, ...),
// walks it in 32-key halves, no LDS, no barrier, the same (O, m, l) partials and the same combine launch.  A row is now 128 bytes = 8 lanes
// x 16 bytes:
//   lane = (ks = lane >> 3, dc = lane & 7): in step i of a half the lane holds the dc-th 16-byte chunk (16 values) of key 8 i + ks, so a
//   request covers eight whole rows and a half is 4 K + 4 V requests (8 KiB per wave, half the bf16 kernel's).  To keep that kernel's 16 KiB
//   in flight while a half is reduced, the halves go through a ring of THREE register buffers: two halves are outstanding while the third
//   is reduced (96 VGPRs of buffers against the bf16 kernel's 128).  A half's 32 K scales and 32 V scales are ONE 4-byte request per lane
//   (lanes 0-31 key l's K scale, lanes 32-63 key (l - 32)'s V scale), issued in front of the data so that it is back first; a step
//   fetches its key's scales from the lanes that hold them.
//   score: 16-element partial dot in fp32 on the converted bytes (v_cvt_pk_f32_fp8), summed over the key's 8 lanes (DPP), THEN times the
//   key's scale -- once per key, not per element; P.V: the probability is multiplied by the V row's scale once, then 16 fp32 FMAs.
struct AttnFp8Args {
    const uint16_t* q; KvFp8Cache c;
    int64_t Tk, q_sb, q_sh;
    const int64_t* dyn_pos; float* part_o; float* part_ml;
    int H, n_splits;
    float scale_log2;
};

typedef float fp8_f32x2 __attribute__((ext_vector_type(2)));

__global__ __launch_bounds__(256) void attn_decode_fp8_kernel(AttnFp8Args a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int head = blockIdx.y, bat = blockIdx.z;
    const int split = blockIdx.x * 4 + wave;                 // one split of the key range per wave
    int64_t n_keys = a.Tk;
    if (a.dyn_pos) n_keys = a.dyn_pos[bat] + 1;              // the query at position p sees keys [0, p]
    const int nblk = (int)((n_keys + 63) >> 6);
    const int ks = lane >> 3, dc = lane & 7;
    float qf[16];
    {
        const uint4* qp = (const uint4*)(a.q + bat * a.q_sb + head * a.q_sh);
        fp8_unpack8(qp[2 * dc], qf);
        fp8_unpack8(qp[2 * dc + 1], qf + 8);
    }
    // wave-uniform base + 32-bit lane offset (the host checks Tk * d_st < 4 GiB)
    typedef const __attribute__((address_space(1))) unsigned char* gptr_t;
    const gptr_t kp = (gptr_t)(uint64_t)(a.c.data + bat * a.c.d_sb + head * a.c.d_sh);
    const gptr_t vp = kp + a.c.d_sw;
    const float* __restrict__ sp = a.c.scale + bat * a.c.s_sb + head * a.c.s_sh + (lane < 32 ? 0 : a.c.s_sw);
    const uint32_t tst = (uint32_t)a.c.d_st, dco = (uint32_t)dc * 16;
    typedef unsigned int attn_u32x4 __attribute__((ext_vector_type(4)));
    auto ld16 = [](gptr_t base, uint32_t off) {
        const attn_u32x4 t = *(const __attribute__((address_space(1))) attn_u32x4*)(base + off);
        return make_uint4(t[0], t[1], t[2], t[3]);
    };
    float m_run = -INFINITY, l_run = 0.f;
    float o[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) o[e] = 0.f;
    // the bf16 kernel's walk: half jh of this wave is half (jh & 1) of its block number (jh >> 1)
    const int nhalf = (int)((n_keys + 31) >> 5);
    const int nb_my = split < nblk ? (nblk - split + a.n_splits - 1) / a.n_splits : 0;
    auto half_of = [&](int jh) { return 2 * (split + (jh >> 1) * a.n_splits) + (jh & 1); };
    int n_my = 2 * nb_my;
    if (n_my > 0 && half_of(n_my - 1) >= nhalf) --n_my;     // the last block's second half may lie beyond the keys
    auto load_half = [&](int jh, uint4 (&kr)[4], uint4 (&vr)[4], float& scl) {
        const int64_t base = (int64_t)half_of(jh) * 32;
        int64_t sk = base + (lane & 31);
        sk = sk < n_keys ? sk : n_keys - 1;                  // a ragged last half re-reads the last key (masked below)
        scl = sp[sk];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int64_t key = base + 8 * i + ks;
            key = key < n_keys ? key : n_keys - 1;
            kr[i] = ld16(kp, (uint32_t)key * tst + dco);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            int64_t key = base + 8 * i + ks;
            key = key < n_keys ? key : n_keys - 1;
            vr[i] = ld16(vp, (uint32_t)key * tst + dco);
        }
    };
    auto reduce_half = [&](int jh, const uint4 (&kr)[4], const uint4 (&vr)[4], float scl) {
        const int64_t k0 = (int64_t)half_of(jh) * 32 + ks;
        float sc[4];
        float mb = -INFINITY;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t w[4] = {kr[i].x, kr[i].y, kr[i].z, kr[i].w};
            float d0 = 0.f, d1 = 0.f;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const fp8_f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[u], false);
                const fp8_f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[u], true);
                d0 = fmaf(lo[0], qf[4 * u], d0);
                d1 = fmaf(lo[1], qf[4 * u + 1], d1);
                d0 = fmaf(hi[0], qf[4 * u + 2], d0);
                d1 = fmaf(hi[1], qf[4 * u + 3], d1);
            }
            float d = d0 + d1;
            d += dpp_fetch<EVO_DPP_XOR1>(d);
            d += dpp_fetch<EVO_DPP_XOR2>(d);
            d += dpp_fetch<EVO_DPP_HALF_MIRROR>(d);
            const float s_k = __shfl(scl, 8 * i + ks, 64);
            sc[i] = k0 + 8 * i < n_keys ? d * s_k * a.scale_log2 : -INFINITY;
            mb = fmaxf(mb, sc[i]);
        }
        mb = fmaxf(mb, __shfl_xor(mb, 8, 64));
        mb = fmaxf(mb, __shfl_xor(mb, 16, 64));
        mb = fmaxf(mb, __shfl_xor(mb, 32, 64));
        const float m_new = fmaxf(m_run, mb);                // finite: the half holds at least one key
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        l_run *= alpha;
#pragma unroll
        for (int e = 0; e < 16; ++e) o[e] *= alpha;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float pw = __builtin_amdgcn_exp2f(sc[i] - m_new);
            l_run += pw;
            const float pv = pw * __shfl(scl, 32 + 8 * i + ks, 64);
            const uint32_t w[4] = {vr[i].x, vr[i].y, vr[i].z, vr[i].w};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const fp8_f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[u], false);
                const fp8_f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w[u], true);
                o[4 * u] = fmaf(pv, lo[0], o[4 * u]);
                o[4 * u + 1] = fmaf(pv, lo[1], o[4 * u + 1]);
                o[4 * u + 2] = fmaf(pv, hi[0], o[4 * u + 2]);
                o[4 * u + 3] = fmaf(pv, hi[1], o[4 * u + 3]);
            }
        }
        m_run = m_new;
    };
    {
        uint4 kA[4], vA[4], kB[4], vB[4], kC[4], vC[4];
        float sA = 0.f, sB = 0.f, sC = 0.f;
        if (n_my > 0) load_half(0, kA, vA, sA);
        if (n_my > 1) load_half(1, kB, vB, sB);
        for (int jh = 0; jh < n_my; jh += 3) {               // three halves per trip: the ring turns without register copies
            if (jh + 2 < n_my) load_half(jh + 2, kC, vC, sC);
            reduce_half(jh, kA, vA, sA);
            if (jh + 1 < n_my) {
                if (jh + 3 < n_my) load_half(jh + 3, kA, vA, sA);
                reduce_half(jh + 1, kB, vB, sB);
                if (jh + 2 < n_my) {
                    if (jh + 4 < n_my) load_half(jh + 4, kB, vB, sB);
                    reduce_half(jh + 2, kC, vC, sC);
                }
            }
        }
    }
    // the eight key groups of the wave meet (every lane of a group carries the same l)
    l_run += __shfl_xor(l_run, 8, 64);
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        o[e] += __shfl_xor(o[e], 8, 64);
        o[e] += __shfl_xor(o[e], 16, 64);
        o[e] += __shfl_xor(o[e], 32, 64);
    }
    if (split < a.n_splits) {
        const int64_t slot = ((int64_t)bat * a.H + head) * a.n_splits + split;
        if (ks == 0) {
            float4* po = (float4*)(a.part_o + slot * DH + dc * 16);
            po[0] = make_float4(o[0], o[1], o[2], o[3]);
            po[1] = make_float4(o[4], o[5], o[6], o[7]);
            po[2] = make_float4(o[8], o[9], o[10], o[11]);
            po[3] = make_float4(o[12], o[13], o[14], o[15]);
        }
        if (lane == 0) { a.part_ml[slot * 2] = m_run; a.part_ml[slot * 2 + 1] = l_run; }
    }
}

// ---- host entries ------------------------------------------------------------------------------------------------------------------
static int fp8_misaligned(const void* p, uintptr_t align) { return ((uintptr_t)p & (align - 1)) != 0; }

// the cache operand: non-null, 16-byte aligned data with byte strides that are multiples of 16, 4-byte aligned scales
static int fp8_cache_args(KvFp8Cache& c, void* data, float* scale, int64_t d_sb, int64_t d_st, int64_t d_sw, int64_t d_sh,
                          int64_t s_sb, int64_t s_sw, int64_t s_sh) {
    if (!data || !scale || fp8_misaligned(data, 16) || fp8_misaligned(scale, 4)) return -1;
    if ((d_sb % 16) || (d_st % 16) || (d_sw % 16) || (d_sh % 16) || d_sb < 0 || d_st < 128 || d_sw < 128 || d_sh < 128) return -1;
    if (s_sb < 0 || s_sw < 1 || s_sh < 1) return -1;
    c.data = (uint8_t*)data; c.scale = scale;
    c.d_sb = d_sb; c.d_st = d_st; c.d_sw = d_sw; c.d_sh = d_sh;
    c.s_sb = s_sb; c.s_sw = s_sw; c.s_sh = s_sh;
    return 0;
}

extern "C" int evo_kv_quant_fp8(const void* k, const void* v, void* kv_data, float* kv_scale, int64_t B, int64_t T, int64_t H,
                                int64_t t0, int64_t cap, int64_t k_sb, int64_t k_st, int64_t k_sh, int64_t v_sb, int64_t v_st,
                                int64_t v_sh, int64_t d_sb, int64_t d_st, int64_t d_sw, int64_t d_sh, int64_t s_sb, int64_t s_sw,
                                int64_t s_sh, void* stream) {
    if (B <= 0 || T <= 0 || H <= 0 || t0 < 0 || cap <= 0 || t0 > cap - T || !k || !v) return -1;
    if (T > 0x7fffffff || H > 65535 || B > 65535) return -1;
    if (fp8_misaligned(k, 16) || fp8_misaligned(v, 16)) return -1;
    if ((k_sb % 8) || (k_st % 8) || (k_sh % 8) || (v_sb % 8) || (v_st % 8) || (v_sh % 8)) return -1;      // 16-byte row accesses
    KvFp8Cache c;
    if (fp8_cache_args(c, kv_data, kv_scale, d_sb, d_st, d_sw, d_sh, s_sb, s_sw, s_sh)) return -1;
    const int64_t n_rows = B * T * 2 * H;
    const int64_t grid = (n_rows + 15) / 16;
    if (grid > 0x7fffffff) return -1;
    hipLaunchKernelGGL(kv_quant_fp8_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, (const uint16_t*)k,
                       (const uint16_t*)v, c, n_rows, (int)T, (int)H, t0, k_sb, k_st, k_sh, v_sb, v_st, v_sh);
    return evo_launch_status();
}

extern "C" int evo_rope_append_decode_fp8(void* qkv, void* kv_data, float* kv_scale, const int64_t* pos, const float* inv_freq,
                                          float scaling, int64_t B, int64_t H, int64_t hd, int64_t d_sb, int64_t d_st, int64_t d_sw,
                                          int64_t d_sh, int64_t s_sb, int64_t s_sw, int64_t s_sh, float q_scale, void* stream) {
    if (B <= 0 || H <= 0 || hd != 128 || !qkv || !pos || !inv_freq || !(scaling > 0.f) || !(q_scale > 0.f)) return -1;
    if (fp8_misaligned(qkv, 16) || fp8_misaligned(pos, 8) || fp8_misaligned(inv_freq, 4)) return -1;
    KvFp8Cache c;
    if (fp8_cache_args(c, kv_data, kv_scale, d_sb, d_st, d_sw, d_sh, s_sb, s_sw, s_sh)) return -1;
    if (B * H * (hd / 16) > 0x7fffffff) return -1;
    const int total = (int)(B * H * (hd / 16));
    hipLaunchKernelGGL(rope_append_decode_fp8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (uint4*)qkv, c, pos, inv_freq, scaling, (int)B, (int)H, q_scale);
    return evo_launch_status();
}

extern "C" int evo_attn_decode_fp8(const void* q, const void* kv_data, const float* kv_scale, void* o, int64_t B, int64_t H,
                                   int64_t Tk, int64_t q_sb, int64_t q_sh, int64_t d_sb, int64_t d_st, int64_t d_sw, int64_t d_sh,
                                   int64_t s_sb, int64_t s_sw, int64_t s_sh, const int64_t* dyn_pos, float* part_o, float* part_ml,
                                   int64_t n_splits, float softmax_scale, void* stream) {
    if (B <= 0 || H <= 0 || Tk <= 0 || n_splits <= 0 || n_splits > 1024 || !q || !o || !part_o || !part_ml) return -1;
    if (H > 65535 || B > 65535 || (q_sb % 8) || (q_sh % 8)) return -1;
    if (fp8_misaligned(q, 16) || fp8_misaligned(o, 16) || fp8_misaligned(part_o, 16) || fp8_misaligned(part_ml, 4) ||
        fp8_misaligned(dyn_pos, 8))
        return -1;
    AttnFp8Args a;
    if (fp8_cache_args(a.c, (void*)kv_data, (float*)kv_scale, d_sb, d_st, d_sw, d_sh, s_sb, s_sw, s_sh)) return -1;
    // streaming form only: a key is addressed by a 32-bit byte offset from the (batch, head) base
    if (d_st > 0xffffffffll / Tk || Tk * d_st >= 0xffffffffll) return -1;
    a.q = (const uint16_t*)q; a.Tk = Tk; a.q_sb = q_sb; a.q_sh = q_sh;
    a.dyn_pos = dyn_pos; a.part_o = part_o; a.part_ml = part_ml; a.H = (int)H; a.n_splits = (int)n_splits;
    a.scale_log2 = softmax_scale <= 0.f ? 1.0f : softmax_scale * 1.4426950408889634f;      // <= 0: the queries are pre-scaled
    hipLaunchKernelGGL(attn_decode_fp8_kernel, dim3((unsigned)((n_splits + 3) / 4), (unsigned)H, (unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, a);
    return evo_attn_decode_combine_launch(part_o, part_ml, o, B, H, n_splits, stream);
}
