// k-mer repeat control for the decode pool (the written specification is evo_amd/sh/sample.py: repeat_fold,
// repeat_ended, repeat_penalise, repeat_row).  One launch in front of the sampler launch of the job-control path: per active row it folds
// the token the step is fed into the row's k-mer counts, may end the row's job, and otherwise writes the f32 row the sampler draws from --
// the model's row minus a level on every alphabet symbol, chosen by how often the k-mer that symbol would complete has been seen.
// One 64-lane wave per row, as the sampler kernels.  A row's state is a handful of integers and at most 9 table cells, the same for every
// lane: the wave reads them as uniform values in two rounds of independent loads (what does not depend on the window; then the cells), does
// the integer work in registers, and lane 0 stores what changed -- every load of the state stands before the first store.  The launch is
// latency-bound whatever does it.  No LDS, no atomics, plain vector stores, no host reads, no allocation: capturable.  The arithmetic on
// the row is ONE f32 subtraction per symbol, so there is nothing for the compiler to contract and nothing to round differently.
// Entry point and contract: include/evo_mi355x.h.
#include "common.h"
#include "../../include/evo_mi355x.h"

struct RepeatAlphabet {
    int32_t n_sym;
    int32_t id[EVO_REPEAT_MAX_SYMBOLS];
};

__global__ __launch_bounds__(64) void repeat_rows_kernel(const void* __restrict__ logits, int logits_f32, int64_t ld, float* __restrict__ out,
                                                         const int64_t* __restrict__ fed_ids, uint8_t* active, int32_t* counts, int32_t* ctx,
                                                         int64_t* stat, const float* __restrict__ levels, const int32_t* __restrict__ end_num,
                                                         int64_t end_min_tokens, const int64_t* __restrict__ count, int64_t* length,
                                                         uint8_t* finish, const RepeatAlphabet alpha, int32_t k, int32_t M, int32_t Mk1) {
    const int64_t s = blockIdx.x;
    const int lane = threadIdx.x;
    if (!active[s]) return;
    const int n_sym = alpha.n_sym;

    // ---- round 1: the row (ids lane * 8 .. lane * 8 + 7, widened to f32: exact) and the row's state -- uniform over the wave
    float x[8];
    if (logits_f32) {
        const f32x4_t* p = (const f32x4_t*)((const float*)logits + s * ld) + 2 * lane;
        const f32x4_t a = p[0], b = p[1];
        x[0] = a[0]; x[1] = a[1]; x[2] = a[2]; x[3] = a[3];
        x[4] = b[0]; x[5] = b[1]; x[6] = b[2]; x[7] = b[3];
    } else {
        const uint4 v = ((const uint4*)((const uint16_t*)logits + s * ld))[lane];
        unpack8(v, x);
    }
    int32_t code = ctx[2 * s], len = ctx[2 * s + 1];
    int64_t n_gen = stat[2 * s], rep = stat[2 * s + 1];
    const bool fold = fed_ids != nullptr;
    const int64_t tok = fold ? fed_ids[s] : -1;
    const int64_t en = end_num ? (int64_t)end_num[s] : 0;
    const int64_t cnt = end_num ? count[s] : 0;
    float lv[EVO_REPEAT_LEVELS];
#pragma unroll
    for (int j = 0; j < EVO_REPEAT_LEVELS; ++j) lv[j] = levels[s * EVO_REPEAT_LEVELS + j];
    if (len < 0 || len > k - 1 || code < 0 || code >= Mk1) code = len = 0;        // a window outside its invariants reads as empty: idx < M always

    // ---- the fold, in registers: `hit` is the k-mer the fed token completes (-1: none)
    int32_t hit = -1;
    if (fold) {
        int a = -1;
#pragma unroll
        for (int b = 0; b < EVO_REPEAT_MAX_SYMBOLS; ++b)
            if (b < n_sym && (int64_t)alpha.id[b] == tok) a = b;
        if (a < 0) {
            code = 0;
            len = 0;
        } else if (len == k - 1) {
            hit = code * n_sym + a;                                   // code < Mk1: hit < Mk1 * n_sym = M
            code = hit % Mk1;
        } else {
            code = code * n_sym + a;
            ++len;
        }
        ++n_gen;
    }

    // ---- round 2: the cell the fold completes and the n_sym neighbouring cells the next token could complete.  Every load of the row's
    // state stands before the first store; the one cell that is both written and read again (a homopolymer run) is taken from `hit_count`
    int32_t* row = counts + s * (int64_t)M;
    const bool full = len == k - 1;
    int32_t hit_count = 0;
    if (hit >= 0) {
        const int32_t old = row[hit];
        hit_count = old < 0x7fffffff ? old + 1 : 0x7fffffff;
        if (old >= 1) ++rep;
    }
    int32_t c[EVO_REPEAT_MAX_SYMBOLS];
#pragma unroll
    for (int a = 0; a < EVO_REPEAT_MAX_SYMBOLS; ++a) c[a] = (full && a < n_sym) ? row[code * n_sym + a] : 0;
    const bool ended = en > 0 && n_gen >= end_min_tokens && rep * 1024 > en * n_gen;

    // ---- the state's stores: lane 0, plain stores
    if (lane == 0) {
        if (hit >= 0) row[hit] = hit_count;
        if (fold) {
            ctx[2 * s] = code;
            ctx[2 * s + 1] = len;
            stat[2 * s] = n_gen;
            stat[2 * s + 1] = rep;
        }
        if (ended) {
            active[s] = 0;
            length[s] = cnt;
            finish[s] = EVO_FINISH_REPEAT;
        }
    }
    if (ended) return;                                                // the row of an ended job is not written: the sampler skips it

    // ---- the penalty: ONE f32 subtraction on each symbol's logit, in the lane that holds it
    if (full) {
#pragma unroll
        for (int a = 0; a < EVO_REPEAT_MAX_SYMBOLS; ++a) {
            if (a < n_sym && (alpha.id[a] >> 3) == lane) {
                const int32_t seen = code * n_sym + a == hit ? hit_count : c[a];
                const int q = min(max(seen, 0), EVO_REPEAT_LEVELS - 1);
                float pen = lv[0];
#pragma unroll
                for (int j = 1; j < EVO_REPEAT_LEVELS; ++j)
                    if (j == q) pen = lv[j];
                const int e = alpha.id[a] & 7;
#pragma unroll
                for (int j = 0; j < 8; ++j)
                    if (j == e) x[j] = x[j] - pen;
            }
        }
    }
    f32x4_t* o = (f32x4_t*)(out + s * EVO_REPEAT_V) + 2 * lane;
    o[0] = f32x4_t{x[0], x[1], x[2], x[3]};
    o[1] = f32x4_t{x[4], x[5], x[6], x[7]};
}

extern "C" int evo_repeat_rows_f32(const void* logits, int64_t logits_f32, int64_t ld, float* out, const int64_t* fed_ids, uint8_t* active,
                                   int32_t* counts, int32_t* ctx, int64_t* stat, const float* levels, const int32_t* end_num,
                                   int64_t end_min_tokens, const int64_t* count, int64_t* length, uint8_t* finish, const int32_t* alphabet,
                                   int64_t n_sym, int64_t k, int64_t M, int64_t S, int64_t V, void* stream) {
    if (!logits || !out || !active || !counts || !ctx || !stat || !levels || !alphabet) return -1;
    if (S < 1 || S > 0x7fffffff || V != EVO_REPEAT_V || ld < V || ld % 8 != 0) return -1;
    if (((uintptr_t)logits & 15) || ((uintptr_t)out & 15)) return -1;
    if (((uintptr_t)counts & 3) || ((uintptr_t)ctx & 3) || ((uintptr_t)levels & 3) || ((uintptr_t)end_num & 3)) return -1;
    if (((uintptr_t)stat & 7) || ((uintptr_t)fed_ids & 7) || ((uintptr_t)count & 7) || ((uintptr_t)length & 7)) return -1;
    if (end_num && (!count || !length || !finish || end_min_tokens < 1)) return -1;
    if (n_sym < 1 || n_sym > EVO_REPEAT_MAX_SYMBOLS || k < 1 || k > 0x7fffffff || M < 1 || M > EVO_REPEAT_MAX_TABLE) return -1;
    int64_t p = 1;                                                    // M == n_sym ** k (one symbol: 1 at every k)
    for (int64_t i = 0; n_sym > 1 && i < k && p <= EVO_REPEAT_MAX_TABLE; ++i) p *= n_sym;
    if (p != M) return -1;
    RepeatAlphabet alpha;
    alpha.n_sym = (int32_t)n_sym;
    for (int a = 0; a < EVO_REPEAT_MAX_SYMBOLS; ++a) alpha.id[a] = -1;
    for (int a = 0; a < n_sym; ++a) {                                 // a host array: read here, before the launch
        const int32_t id = alphabet[a];
        if (id < 0 || id >= EVO_REPEAT_V) return -1;
        for (int b = 0; b < a; ++b)
            if (alpha.id[b] == id) return -1;
        alpha.id[a] = id;
    }
    hipLaunchKernelGGL(repeat_rows_kernel, dim3((unsigned)S), dim3(64), 0, (hipStream_t)stream, logits, (int)(logits_f32 != 0), ld, out,
                       fed_ids, active, counts, ctx, stat, levels, end_num, end_min_tokens, count, length, finish, alpha, (int32_t)k,
                       (int32_t)M, (int32_t)(M / n_sym));
    return evo_launch_status();
}
