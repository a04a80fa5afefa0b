// Paged bf16 KV cache for the decode pool (include/evo_mi355x.h): the append and the decode attention that find a
// stream's keys through a page table instead of one contiguous run per stream.
//
// Layout of a layer: pages [n_pages, page_tokens, 2, H, 128] bf16 -- inside a page the contiguous cache's layout -- and ONE table
// [B, table_width] int32 for all layers: token t of stream b lives in page table[b, t >> log2(page_tokens)] at row t & (page_tokens - 1).
// page_tokens is a power of two >= 64, so a 64-key block of the streaming kernel (and each of its 32-key halves) lies inside one page.
// Page 0 is a scrap page: every table entry no live job owns holds 0, so idle rows append into and read from page 0 only.
//
// Both kernels are their contiguous siblings (attn_decode_stream_kernel in csrc/attn.hip, rope_append_decode_kernel in
// csrc/elementwise.hip) statement for statement in everything that produces a value; only the addresses differ.  Whatever the table holds,
// no access leaves the page pool: a table index is clamped to [0, table_width - 1] and a page id to [0, n_pages - 1].
#include "common.h"
#include "../../include/evo_mi355x.h"

#include "attn_common.h"

struct PagedKvArgs {               // the cache operand of both launches
    const int32_t* table;          // [B, table_width]
    int table_width, n_pages, log2_pt;
    int64_t sp, st, sw, sh;        // page, token, k|v, head strides (attention: bytes; append: 16-byte vectors)
};

__device__ __forceinline__ int paged_clamp(int x, int hi) { return x < 0 ? 0 : (x > hi ? hi : x); }

// ---- evo_rope_append_decode_paged_bf16
__global__ __launch_bounds__(256) void rope_append_decode_paged_kernel(uint4* __restrict__ qkv, uint4* __restrict__ pages, PagedKvArgs pk,
                                                                       const int64_t* __restrict__ pos,
                                                                       const float* __restrict__ inv_freq, float scaling, int B,
                                                                       int H, int hd, float q_scale) {
    const int half_vec = hd / 16;
    const int total = B * H * half_vec;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
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
    // the cache row written: page table[b, p >> log2(page_tokens)], row p & (page_tokens - 1) of it
    const int64_t te = p >> pk.log2_pt;
    const int ti = te < 0 ? 0 : (te > pk.table_width - 1 ? pk.table_width - 1 : (int)te);
    const int64_t pg = paged_clamp(pk.table[(int64_t)b * pk.table_width + ti], pk.n_pages - 1);
    const int64_t w = p & (((int64_t)1 << pk.log2_pt) - 1);
    uint4* krow = pages + pg * pk.sp + w * pk.st + h * pk.sh;
    uint4* vrow = krow + pk.sw;
#pragma unroll
    for (int which = 0; which < 2; ++which) {                // q, k
        const int64_t row_vec = (((int64_t)b * 3 + which) * H + h) * rv;
        float x0[8], x1[8], o0[8], o1[8];
        unpack8(qkv[row_vec + c], x0);
        unpack8(qkv[row_vec + half_vec + c], x1);
        const float qs = which == 0 ? q_scale : 1.0f;         // (see rope_kernel)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            o0[e] = (x0[e] * co[e] - x1[e] * si[e]) * qs;
            o1[e] = (x0[e] * si[e] + x1[e] * co[e]) * qs;
        }
        const uint4 r0 = pack8(o0), r1 = pack8(o1);
        qkv[row_vec + c] = r0;
        qkv[row_vec + half_vec + c] = r1;
        if (which == 1) { krow[c] = r0; krow[half_vec + c] = r1; }
    }
    const int64_t vvec = (((int64_t)b * 3 + 2) * H + h) * rv;
    vrow[c] = qkv[vvec + c];
    vrow[half_vec + c] = qkv[vvec + half_vec + c];
}

// ---- evo_attn_decode_paged_bf16: attn_decode_stream_kernel with a page lookup per 64-key block.  A wave's blocks (split, split + n_splits,
// ...) are known before its loop, so their page ids are taken AHEAD of use: lane l holds the page id of the wave's (64 c + l)-th block
// (one 4-byte load per lane and 64 blocks, issued before the first K/V request of those blocks), and a half's wave-uniform 64-bit base is
// pages + readlane(id) * page stride + head offset.  The lane's 32-bit offset is (key & (page_tokens - 1)) * token stride + dc * 16.  No
// load sits under a per-element condition.
struct AttnPagedArgs {
    const uint16_t* q; const unsigned char* pages; PagedKvArgs pk;
    int64_t q_sb, q_sh;
    const int64_t* dyn_pos; float* part_o; float* part_ml;
    int H, n_splits;
    float scale_log2;
};

__global__ __launch_bounds__(256) void attn_decode_paged_kernel(AttnPagedArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int head = blockIdx.y, bat = blockIdx.z;
    const int split = blockIdx.x * 4 + wave;                 // one split of the key range per wave
    const int64_t n_keys = a.dyn_pos[bat] + 1;               // the query at position p sees keys [0, p]
    const int nblk = (int)((n_keys + 63) >> 6);
    const int ks = lane >> 4, dc = lane & 15;
    const uint4 qv = ((const uint4*)(a.q + bat * a.q_sb + head * a.q_sh))[dc];
    typedef const __attribute__((address_space(1))) unsigned char* gptr_t;
    const uint64_t base0 = (uint64_t)(a.pages + head * a.pk.sh);
    const uint64_t psp = (uint64_t)a.pk.sp, psw = (uint64_t)a.pk.sw;
    const uint32_t tst = (uint32_t)a.pk.st, dco = (uint32_t)dc * 16;
    const int64_t pmask = ((int64_t)1 << a.pk.log2_pt) - 1;
    const int bshift = a.pk.log2_pt - 6;                     // 64-key block -> table entry
    const int32_t* __restrict__ trow = a.pk.table + (int64_t)bat * a.pk.table_width;
    typedef unsigned int attn_u32x4 __attribute__((ext_vector_type(4)));
    auto ld16 = [](gptr_t base, uint32_t off) {
        const attn_u32x4 t = *(const __attribute__((address_space(1))) attn_u32x4*)(base + off);
        return make_uint4(t[0], t[1], t[2], t[3]);
    };
    float m_run = -INFINITY, l_run = 0.f;
    float o[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = 0.f;
    const int nhalf = (int)((n_keys + 31) >> 5);
    const int nb_my = split < nblk ? (nblk - split + a.n_splits - 1) / a.n_splits : 0;
    auto half_of = [&](int jh) { return 2 * (split + (jh >> 1) * a.n_splits) + (jh & 1); };
    int n_my = 2 * nb_my;
    if (n_my > 0 && half_of(n_my - 1) >= nhalf) --n_my;     // the last block's second half may lie beyond the keys
    // page ids of this wave's blocks 64 c .. 64 c + 63, one per lane (every lane loads: an index past the table is clamped into it)
    auto page_ids = [&](int c) {
        const int64_t blk = (int64_t)split + (int64_t)(64 * c + lane) * a.n_splits;
        const int64_t te = blk >> bshift;
        const int ti = te > a.pk.table_width - 1 ? a.pk.table_width - 1 : (int)te;
        return paged_clamp(trow[ti], a.pk.n_pages - 1);
    };
    // (a wave without blocks asks for none: behind short prompts most of a row's waves are such, and the lookup was their whole run time)
    int pg = nb_my > 0 ? page_ids(0) : 0;
    auto load_half = [&](int jh, uint4 (&kr)[8], uint4 (&vr)[8]) {
        const int64_t k0 = (int64_t)half_of(jh) * 32 + ks;
        const uint64_t pbase = base0 + (uint64_t)(uint32_t)__builtin_amdgcn_readlane(pg, (jh >> 1) & 63) * psp;
        const gptr_t kp = (gptr_t)pbase, vp = (gptr_t)(pbase + psw);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int64_t key = k0 + 4 * i;
            key = key < n_keys ? key : n_keys - 1;           // a ragged last half re-reads the last key (masked below): same half, same page
            kr[i] = ld16(kp, (uint32_t)(key & pmask) * tst + dco);
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int64_t key = k0 + 4 * i;
            key = key < n_keys ? key : n_keys - 1;
            vr[i] = ld16(vp, (uint32_t)(key & pmask) * tst + dco);
        }
    };
    auto reduce_half = [&](int jh, const uint4 (&kr)[8], const uint4 (&vr)[8]) {
        const int64_t k0 = (int64_t)half_of(jh) * 32 + ks;
        float sc[8];
        float mb = -INFINITY;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            float d = attn_dot8(kr[i], qv);
            d += __shfl_xor(d, 1, 64);
            d += __shfl_xor(d, 2, 64);
            d += __shfl_xor(d, 4, 64);
            d += __shfl_xor(d, 8, 64);
            sc[i] = k0 + 4 * i < n_keys ? d * a.scale_log2 : -INFINITY;
            mb = fmaxf(mb, sc[i]);
        }
        mb = fmaxf(mb, __shfl_xor(mb, 16, 64));
        mb = fmaxf(mb, __shfl_xor(mb, 32, 64));
        const float m_new = fmaxf(m_run, mb);                // finite: the half holds at least one key
        const float alpha = __builtin_amdgcn_exp2f(m_run - m_new);
        l_run *= alpha;
#pragma unroll
        for (int e = 0; e < 8; ++e) o[e] *= alpha;
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const float pw = __builtin_amdgcn_exp2f(sc[i] - m_new);
            l_run += pw;
            o[0] = fmaf(pw, bf_lo(vr[i].x), o[0]); o[1] = fmaf(pw, bf_hi(vr[i].x), o[1]);
            o[2] = fmaf(pw, bf_lo(vr[i].y), o[2]); o[3] = fmaf(pw, bf_hi(vr[i].y), o[3]);
            o[4] = fmaf(pw, bf_lo(vr[i].z), o[4]); o[5] = fmaf(pw, bf_hi(vr[i].z), o[5]);
            o[6] = fmaf(pw, bf_lo(vr[i].w), o[6]); o[7] = fmaf(pw, bf_hi(vr[i].w), o[7]);
        }
        m_run = m_new;
    };
    {
        uint4 kA[8], vA[8], kB[8], vB[8];
        if (n_my > 0) load_half(0, kA, vA);
        for (int jh = 0; jh < n_my; jh += 2) {               // two halves per trip: the buffers alternate without register copies
            if (jh + 1 < n_my) load_half(jh + 1, kB, vB);
            reduce_half(jh, kA, vA);
            if (jh + 1 < n_my) {
                if (jh + 2 < n_my) {
                    // the next block starts another run of 64: its ids (once per 64 blocks of a wave, i.e. per 2 MiB it streams)
                    if (((jh + 2) & 127) == 0) pg = page_ids((jh + 2) >> 7);
                    load_half(jh + 2, kA, vA);
                }
                reduce_half(jh + 1, kB, vB);
            }
        }
    }
    // the four key groups of the wave meet (every lane of a group carries the same l)
    l_run += __shfl_xor(l_run, 16, 64);
    l_run += __shfl_xor(l_run, 32, 64);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        o[e] += __shfl_xor(o[e], 16, 64);
        o[e] += __shfl_xor(o[e], 32, 64);
    }
    if (split < a.n_splits) {
        const int64_t slot = ((int64_t)bat * a.H + head) * a.n_splits + split;
        if (ks == 0) {
            float4* po = (float4*)(a.part_o + slot * DH + dc * 8);
            po[0] = make_float4(o[0], o[1], o[2], o[3]);
            po[1] = make_float4(o[4], o[5], o[6], o[7]);
        }
        if (lane == 0) { a.part_ml[slot * 2] = m_run; a.part_ml[slot * 2 + 1] = l_run; }
    }
}

// ---- host entries ------------------------------------------------------------------------------------------------------------------
static int paged_misaligned(const void* p, uintptr_t align) { return ((uintptr_t)p & (align - 1)) != 0; }

// the cache operand: non-null 16-byte aligned pages, a 4-byte aligned table, page_tokens a power of two >= 64 whose span in one page
// stays below 4 GiB (the lane's 32-bit offset), element strides that keep every row access 16-byte aligned.  Strides leave in bytes.
static int paged_cache_args(PagedKvArgs& pk, const void* pages, const void* table, int64_t page_tokens, int64_t n_pages,
                            int64_t table_width, int64_t sp, int64_t st, int64_t sw, int64_t sh) {
    if (!pages || !table || paged_misaligned(pages, 16) || paged_misaligned(table, 4)) return -1;
    if (page_tokens < 64 || (page_tokens & (page_tokens - 1)) || page_tokens > ((int64_t)1 << 30)) return -1;
    if (n_pages < 1 || n_pages > 0x7fffffff || table_width < 1 || table_width > 0x7fffffff) return -1;
    if ((sp % 8) || (st % 8) || (sw % 8) || (sh % 8) || sp < 0 || st < 128 || sw < 128 || sh < 128) return -1;
    if (st * 2 > 0xffffffffll / page_tokens || page_tokens * st * 2 >= 0xffffffffll) return -1;
    int l = 0;
    while (((int64_t)1 << l) < page_tokens) ++l;
    pk.table = (const int32_t*)table; pk.table_width = (int)table_width; pk.n_pages = (int)n_pages; pk.log2_pt = l;
    pk.sp = sp * 2; pk.st = st * 2; pk.sw = sw * 2; pk.sh = sh * 2;
    return 0;
}

extern "C" int evo_rope_append_decode_paged_bf16(void* qkv, void* pages, const int32_t* table, const int64_t* pos, const float* inv_freq,
                                                 float scaling, int64_t B, int64_t H, int64_t hd, int64_t page_tokens, int64_t n_pages,
                                                 int64_t table_width, int64_t p_sp, int64_t p_st, int64_t p_sw, int64_t p_sh,
                                                 float q_scale, void* stream) {
    if (B <= 0 || H <= 0 || hd != 128 || !qkv || !pos || !inv_freq || !(scaling > 0.f) || !(q_scale > 0.f)) return -1;
    if (paged_misaligned(qkv, 16) || paged_misaligned(pos, 8) || paged_misaligned(inv_freq, 4)) return -1;
    PagedKvArgs pk;
    if (paged_cache_args(pk, pages, table, page_tokens, n_pages, table_width, p_sp, p_st, p_sw, p_sh)) return -1;
    if (B * H * (hd / 16) > 0x7fffffff) return -1;
    pk.sp /= 16; pk.st /= 16; pk.sw /= 16; pk.sh /= 16;      // the append addresses 16-byte vectors, as its sibling does
    const int total = (int)(B * H * (hd / 16));
    hipLaunchKernelGGL(rope_append_decode_paged_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (uint4*)qkv, (uint4*)pages, pk, pos, inv_freq, scaling, (int)B, (int)H, (int)hd, q_scale);
    return evo_launch_status();
}

extern "C" int evo_attn_decode_paged_bf16(const void* q, const void* pages, const int32_t* table, void* o, int64_t B, int64_t H,
                                          int64_t page_tokens, int64_t n_pages, int64_t table_width, int64_t q_sb, int64_t q_sh,
                                          int64_t p_sp, int64_t p_st, int64_t p_sw, int64_t p_sh, const int64_t* pos, float* part_o,
                                          float* part_ml, int64_t n_splits, float softmax_scale, void* stream) {
    if (B <= 0 || H <= 0 || n_splits <= 0 || n_splits > 1024 || !q || !o || !pos || !part_o || !part_ml) return -1;
    if (H > 65535 || B > 65535 || (q_sb % 8) || (q_sh % 8)) return -1;
    if (paged_misaligned(q, 16) || paged_misaligned(o, 16) || paged_misaligned(part_o, 16) || paged_misaligned(part_ml, 4) ||
        paged_misaligned(pos, 8))
        return -1;
    AttnPagedArgs a;
    if (paged_cache_args(a.pk, pages, table, page_tokens, n_pages, table_width, p_sp, p_st, p_sw, p_sh)) return -1;
    a.q = (const uint16_t*)q; a.pages = (const unsigned char*)pages; a.q_sb = q_sb; a.q_sh = q_sh;
    a.dyn_pos = pos; a.part_o = part_o; a.part_ml = part_ml; a.H = (int)H; a.n_splits = (int)n_splits;
    a.scale_log2 = softmax_scale <= 0.f ? 1.0f : softmax_scale * 1.4426950408889634f;      // <= 0: the queries are pre-scaled
    hipLaunchKernelGGL(attn_decode_paged_kernel, dim3((unsigned)((n_splits + 3) / 4), (unsigned)H, (unsigned)B), dim3(256), 0,
                       (hipStream_t)stream, a);
    return evo_attn_decode_combine_launch(part_o, part_ml, o, B, H, n_splits, stream);
}
