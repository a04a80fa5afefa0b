// Beam search on the device (the written specification is evo_amd/sh/sample.py: beam_select).  Two kernels, both
// capturable: no host read, no allocation, no float atomics; every store is a plain vector store from a lane.
//
// beam_select_kernel (evo_beam_select_f32): a prompt owns a GROUP of W <= 8 consecutive slots.  One workgroup per group, one 64-lane
// wave per beam.  Wave b reads its slot's state, computes the log-sum-exp of its row exactly as the sampler does (EVO_SAMPLE_ROW_LSE,
// csrc/sample_row.h) and packs every candidate into a 64-bit key: the score cum[b] + (x - lse) as the order-preserving pattern of
// sample_ord in the high word; (7 - b) << 9 | (511 - token) in the low word -- so "score descending, then parent ascending, then token
// ascending" is ONE unsigned comparison, and key 0 is "no candidate".  W rounds of a wave-wide maximum leave the wave's W best in LDS;
// after ONE barrier wave 0 merges the W x W survivors the same way and lanes 0 ... W - 1 write the group's slots.  Hazard rule: ALL state
// (cum, ended, length, ids of the group's W slots) is read and staged in LDS BEFORE that barrier, and only wave 0 writes, after it; a
// group touches no other group's slots.
//
// gather_rows_kernel (evo_gather_rows): the reparenting copy.  For every slot s with parent[s] != s, row parent[s] of every registered
// tensor goes to row s.  A row about to be overwritten may still be another slot's source, so the copy goes OUT to a scratch row of s
// in one launch and BACK in a second: nothing is read after it may have been written, and nothing is ordered inside a launch.  All
// tensors travel through one device table (EVO_GATHER_FIELDS int64 per entry).
#include "common.h"
#include "sample_row.h"
#include "../../include/evo_mi355x.h"

__device__ __forceinline__ uint64_t beam_wave_max(uint64_t k) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)k, d, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(k >> 32), d, 64);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        k = o > k ? o : k;
    }
    return k;
}

__device__ __forceinline__ uint64_t beam_key(float score, int beam, int field) {
    if (score == 0.f) score = 0.f;                                    // -0 and +0 are one value
    return ((uint64_t)sample_ord(score) << 32) | ((uint32_t)(EVO_BEAM_MAX_WIDTH - 1 - beam) << 9) | (uint32_t)field;
}

__global__ __launch_bounds__(64 * EVO_BEAM_MAX_WIDTH) void beam_select_kernel(
        const void* __restrict__ logits, int logits_f32, int64_t ld, const uint8_t* __restrict__ allow, const uint8_t* __restrict__ stop_mask,
        const uint8_t* __restrict__ group_active, float* cum, uint8_t* ended, int64_t* length, int64_t* ids, int64_t* parent,
        int32_t* hist_parent, int64_t* hist_ids, float* hist_cum, int64_t hist_len, int64_t* step, int64_t t, int W, int64_t S, int64_t G) {
    __shared__ uint64_t keys[EVO_BEAM_MAX_WIDTH * EVO_BEAM_MAX_WIDTH];
    __shared__ int64_t o_len[EVO_BEAM_MAX_WIDTH], o_ids[EVO_BEAM_MAX_WIDTH];
    __shared__ float o_cum[EVO_BEAM_MAX_WIDTH];
    __shared__ int o_end[EVO_BEAM_MAX_WIDTH];
    const int64_t g = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;       // wave < W: the block has 64 W threads
    const int64_t s = g * W + wave;                                   // < G W <= S
    if (g == 0 && (int64_t)threadIdx.x < S - G * W) parent[G * W + threadIdx.x] = G * W + threadIdx.x;      // the leftover slots: fewer than W
    if (group_active && !group_active[g]) {                           // (the whole workgroup: before any barrier)
        if (lane == 0) parent[s] = s;
        return;
    }
    const float c = cum[s];
    const bool was_ended = ended[s] != 0;
    if (lane == 0) {
        o_cum[wave] = c;
        o_end[wave] = was_ended ? 1 : 0;
        o_len[wave] = length[s];
        o_ids[wave] = ids[s];
    }
    uint64_t k[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) k[j] = 0;
    if (c > -INFINITY) {                                              // (wave-uniform; an empty beam -- or a NaN -- offers nothing)
        if (was_ended) {
            if (lane == 0) k[0] = beam_key(c, wave, EVO_SAMPLE_V - 1);                // itself
        } else {
            float x[8];
            if (logits_f32) {
                const f32x4_t* p = (const f32x4_t*)((const float*)logits + s * ld) + 2 * lane;
                const f32x4_t a = p[0], b = p[1];
                x[0] = a[0]; x[1] = a[1]; x[2] = a[2]; x[3] = a[3];
                x[4] = b[0]; x[5] = b[1]; x[6] = b[2]; x[7] = b[3];
            } else {
                unpack8(((const uint4*)((const uint16_t*)logits + s * ld))[lane], x);
            }
            EVO_SAMPLE_ROW_LSE(x, lse)
            const uint32_t abits = allow ? allow[lane] : 0xffu;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float sc = c + (x[j] - lse);
                const bool ok = ((abits >> j) & 1u) && sc > -INFINITY;               // (a NaN compares false)
                k[j] = ok ? beam_key(sc, wave, EVO_SAMPLE_V - 1 - (lane * 8 + j)) : 0;
            }
        }
    }
    for (int r = 0; r < W; ++r) {                                     // the wave's W best, in order; keys are distinct or 0
        uint64_t m = k[0];
#pragma unroll
        for (int j = 1; j < 8; ++j) m = k[j] > m ? k[j] : m;
        m = beam_wave_max(m);
        if (lane == 0) keys[wave * EVO_BEAM_MAX_WIDTH + r] = m;
#pragma unroll
        for (int j = 0; j < 8; ++j) k[j] = k[j] == m ? 0 : k[j];
    }
    __syncthreads();
    if (wave != 0) return;

    // ---- wave 0: the W x W survivors, one per lane (lane = 8 beam + rank)
    uint64_t mine = ((lane >> 3) < W && (lane & 7) < W) ? keys[lane] : 0;
    uint64_t sel = 0;
    for (int j = 0; j < W; ++j) {
        const uint64_t m = beam_wave_max(mine);
        if (lane == j) sel = m;
        mine = mine == m ? 0 : mine;
    }
    const int64_t col = step ? step[g] : t;
    const bool rec = hist_len > 0 && col >= 0 && col < hist_len;
    if (lane < W) {
        const int64_t so = g * W + lane;
        int64_t par = so, tok = o_ids[lane];
        float nc = -INFINITY;
        if (sel != 0) {
            const int b = EVO_BEAM_MAX_WIDTH - 1 - (int)(((uint32_t)sel >> 9) & 7u);   // < W: the key came from wave b
            const bool pe = o_end[b] != 0;
            tok = pe ? o_ids[b] : (int64_t)(EVO_SAMPLE_V - 1 - (int)((uint32_t)sel & 511u));
            nc = pe ? o_cum[b] : sample_unord((uint32_t)(sel >> 32));
            par = g * W + b;
            const bool stop = !pe && stop_mask && ((stop_mask[tok >> 3] >> (tok & 7)) & 1u);
            ids[so] = tok;
            length[so] = o_len[b] + (pe ? 0 : 1);
            ended[so] = (pe || stop) ? 1 : 0;
        } else {
            ended[so] = 0;                                            // empty: ids and length stay
        }
        parent[so] = par;
        cum[so] = nc;
        if (rec) {
            hist_parent[so * hist_len + col] = (int32_t)par;
            hist_ids[so * hist_len + col] = tok;
            if (hist_cum) hist_cum[so * hist_len + col] = nc;
        }
    }
    if (lane == 0 && step) step[g] = col + 1;
}

extern "C" int evo_beam_select_f32(const void* logits, int64_t logits_f32, int64_t ld, const void* allow, const void* stop_mask,
                                   const uint8_t* group_active, float* cum, uint8_t* ended, int64_t* length, int64_t* ids, int64_t* parent,
                                   int32_t* hist_parent, int64_t* hist_ids, float* hist_cum, int64_t hist_len, int64_t* step, int64_t t,
                                   int64_t W, int64_t S, int64_t V, void* stream) {
    if (!logits || !cum || !ended || !length || !ids || !parent) return -1;
    if (W < 1 || W > EVO_BEAM_MAX_WIDTH || S < W || S > 0x7fffffff || V != EVO_SAMPLE_V || ld < V || ld % 8 != 0) return -1;
    if (((uintptr_t)logits & 15) || ((uintptr_t)cum & 3) || ((uintptr_t)length & 7) || ((uintptr_t)ids & 7) || ((uintptr_t)parent & 7)) return -1;
    if (((uintptr_t)hist_parent & 3) || ((uintptr_t)hist_ids & 7) || ((uintptr_t)hist_cum & 3) || ((uintptr_t)step & 7)) return -1;
    if (t >= 0 || step) {                                             // a step to record: the history must be there
        if (!hist_parent || !hist_ids || hist_len < 1) return -1;
    } else {
        hist_parent = nullptr; hist_ids = nullptr; hist_cum = nullptr; hist_len = 0;
    }
    const int64_t G = S / W;
    hipLaunchKernelGGL(beam_select_kernel, dim3((unsigned)G), dim3(64 * (unsigned)W), 0, (hipStream_t)stream, logits, (int)(logits_f32 != 0), ld,
                       (const uint8_t*)allow, (const uint8_t*)stop_mask, group_active, cum, ended, length, ids, parent, hist_parent, hist_ids,
                       hist_cum, hist_len, step, t, (int)W, S, G);
    return evo_launch_status();
}

// ---------------------------------------------------------------------------------------------------------------- the reparenting copy
// Entry e of the table: [0] base address, [1] row stride in bytes, [2] bytes of a row to move (a fixed row: all of them; a per-token row:
// its capacity), [3] bytes per token (0: a fixed row; > 0: only the first own_pos[parent] + 1 tokens move), [4] offset of the entry in a
// scratch row, [5] 0.  Everything is a multiple of 16 bytes (the Python binding builds and checks the table).
__global__ __launch_bounds__(256) void gather_rows_kernel(const int64_t* __restrict__ table, const int64_t* __restrict__ parent,
                                                          const int64_t* __restrict__ own_pos, uint8_t* scratch, int64_t scratch_row_bytes,
                                                          int64_t S, int back) {
    const int64_t s = blockIdx.z;
    int64_t p = parent[s];
    p = p < 0 ? 0 : (p > S - 1 ? S - 1 : p);
    if (p == s) return;                                               // late in a search: most slots
    const int64_t* te = table + (int64_t)blockIdx.y * EVO_GATHER_FIELDS;
    uint8_t* base = (uint8_t*)(uintptr_t)te[0];
    const int64_t stride = te[1], bpt = te[3], off = te[4];
    int64_t n = te[2];
    if (bpt > 0) {
        int64_t live = own_pos[p] + 1;                                // the keys generated so far, this step's append included
        const int64_t cap = n / bpt;
        live = live < 0 ? 0 : (live > cap ? cap : live);
        n = live * bpt;
    }
    if (off < 0 || off >= scratch_row_bytes) return;
    n = n > scratch_row_bytes - off ? scratch_row_bytes - off : n;    // never outside the slot's scratch row
    uint8_t* mine = scratch + s * scratch_row_bytes + off;
    const uint4* src = (const uint4*)(back ? mine : base + p * stride);
    uint4* dst = (uint4*)(back ? base + s * stride : mine);
    const int64_t nvec = n >> 4;
#pragma unroll 4
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * 256) dst[i] = src[i];
}

extern "C" int evo_gather_rows(const int64_t* table, int64_t n_entries, const int64_t* parent, const int64_t* own_pos, void* scratch,
                               int64_t scratch_row_bytes, int64_t max_row_bytes, int64_t S, int64_t back, void* stream) {
    if (!table || !parent || !own_pos || !scratch) return -1;
    if (((uintptr_t)table & 7) || ((uintptr_t)parent & 7) || ((uintptr_t)own_pos & 7) || ((uintptr_t)scratch & 15)) return -1;
    if (n_entries < 1 || n_entries > 65535 || S < 1 || S > 65535) return -1;
    if (scratch_row_bytes < 16 || scratch_row_bytes % 16 != 0 || max_row_bytes < 16 || max_row_bytes % 16 != 0) return -1;
    if (max_row_bytes > scratch_row_bytes || (back != 0 && back != 1)) return -1;
    int64_t bx = (max_row_bytes / 16 + 256 * 8 - 1) / (256 * 8);      // about 8 vectors per lane of the longest row
    bx = bx < 1 ? 1 : (bx > 64 ? 64 : bx);
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)bx, (unsigned)n_entries, (unsigned)S), dim3(256), 0, (hipStream_t)stream, table, parent,
                       own_pos, (uint8_t*)scratch, scratch_row_bytes, S, (int)back);
    return evo_launch_status();
}
