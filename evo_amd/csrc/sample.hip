// Seeded sampling of one token per row of [S, 512] logits, entirely on the device (the written
// specification is evo_amd/sh/sample.py: sample_seeded).  One launch, no host reads, no allocation: capturable in a hipGraph.
// One 64-lane wave per row.  The row's 512 (logit, id) pairs are packed into 64-bit keys -- the logit as an order-preserving
// 32-bit pattern in the high word, 511 - id in the low word -- and sorted DESCENDING by a bitonic network through 4 KB of LDS,
// which gives the order "logit descending, ties by ascending id".  Everything else falls out of that one order, 8 consecutive
// positions per lane: the k-th value (top-k keeps its ties), the top-p cut (the reference's ascending cumulative softmax is the
// suffix sum here, so the survivors are a prefix) and the CDF walk.  Sums are fp32 in a FIXED order (8 sequential terms per lane,
// then a Hillis-Steele scan / butterfly over the lanes), so a row's token is bit-identical from run to run.  No float atomics.
// The random number of a row is Philox4x32-10 keyed by the seed, counter = (stream id, draw count): a function of the sample and
// the draw, not of the slot or the step.  Entry points and contracts: include/evo_mi355x.h.
// Three kernels share the draw (sample_draw_row): sample_rows_kernel (evo_sample_rows_f32) records it and advances the count;
// sample_rows_ctl_kernel (evo_sample_rows_ctl_f32) also decides that the row's job is over -- stop token,
// in-frame stop pattern at the end of the recorded tokens, own length limit -- clears the row's `active` byte and writes `length` /
// `finish`: lane 0, plain stores, a look-back of at most 7 cells into the row's own token history; sample_rows_dfa_kernel
// (evo_sample_rows_dfa_f32) is the control kernel whose allow set at each draw is decided by the row's state in
// a small token automaton, which the drawn token moves on.
#include "common.h"
#include "sample_row.h"     // sample_ord / sample_unord, the wave sum, the log-sum-exp: shared with csrc/beam.hip
#include "../../include/evo_mi355x.h"

__device__ __forceinline__ uint32_t philox4x32_10_x0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        const uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c1 = (uint32_t)p1;
        c3 = (uint32_t)p0;
        c0 = n0;
        c2 = n2;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c0;
}

// The draw of one row by one wave, shared by the kernels below: token and its log-probability under the unfiltered row (every lane
// returns the same pair).  `abits`: the lane's 8 allow bits (sample_allow_bits, or a narrower set).  With `hist_row` the row's 512 f32
// logits are also stored there.  `keys` / `raw`: the workgroup's LDS.
struct SampleDraw { int tok; float logprob; };

// the lane's byte of the 64-byte allow mask (bit j of byte b: token 8 b + j); no mask allows everything
__device__ __forceinline__ uint32_t sample_allow_bits(const uint8_t* __restrict__ allow) {
    return allow ? allow[threadIdx.x] : 0xffu;
}

__device__ __forceinline__ SampleDraw sample_draw_row(const void* __restrict__ logits, int logits_f32, int64_t ld, int64_t s,
                                                      const int32_t* __restrict__ top_k, const float* __restrict__ top_p,
                                                      const float* __restrict__ temperature, const uint32_t abits,
                                                      uint32_t seed_lo, uint32_t seed_hi, int64_t sid, int64_t cnt, float* hist_row,
                                                      uint64_t* keys, float* raw) {
    const int lane = threadIdx.x;

    // ---- the row: ids lane * 8 .. lane * 8 + 7
    float x[8];
    if (logits_f32) {
        const f32x4_t* p = (const f32x4_t*)((const float*)logits + s * ld) + 2 * lane;
        const f32x4_t a = p[0], b = p[1];
        x[0] = a[0]; x[1] = a[1]; x[2] = a[2]; x[3] = a[3];
        x[4] = b[0]; x[5] = b[1]; x[6] = b[2]; x[7] = b[3];
    } else {
        const uint4 v = ((const uint4*)((const uint16_t*)logits + s * ld))[lane];
        x[0] = bf_lo(v.x); x[1] = bf_hi(v.x); x[2] = bf_lo(v.y); x[3] = bf_hi(v.y);
        x[4] = bf_lo(v.z); x[5] = bf_hi(v.z); x[6] = bf_lo(v.w); x[7] = bf_hi(v.w);
    }
    if (hist_row) {
        f32x4_t* h = (f32x4_t*)hist_row + 2 * lane;
        h[0] = f32x4_t{x[0], x[1], x[2], x[3]};
        h[1] = f32x4_t{x[4], x[5], x[6], x[7]};
    }

    // ---- log-sum-exp of the UNFILTERED row (fp32)
    EVO_SAMPLE_ROW_LSE(x, lse)

    // ---- keys: allow bits (bit j of `abits`: token 8 lane + j), then (logit, id) -> LDS
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int id = lane * 8 + j;
        raw[id] = x[j];
        float v = ((abits >> j) & 1u) ? x[j] : -INFINITY;
        if (v == 0.f) v = 0.f;                                        // -0 and +0 are one value
        keys[id] = ((uint64_t)sample_ord(v) << 32) | (uint32_t)(EVO_SAMPLE_V - 1 - id);
    }
    __syncthreads();

    // ---- bitonic sort, descending: 45 steps of 256 compare-exchanges (4 per lane); every index stays below 512
    for (int k = 2; k <= EVO_SAMPLE_V; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int t = lane; t < EVO_SAMPLE_V / 2; t += 64) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));  // bit j clear
                const int p = i | j;
                const uint64_t a = keys[i], b = keys[p];
                const bool down = (i & k) == 0;
                if ((a < b) == down) { keys[i] = b; keys[p] = a; }
            }
            __syncthreads();
        }
    }

    // ---- sorted positions lane * 8 .. lane * 8 + 7
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = sample_unord((uint32_t)(keys[lane * 8 + j] >> 32));
    const float v0 = sample_unord((uint32_t)(keys[0] >> 32));
    const int k = top_k[s];
    int pos = 0;                                                      // top_k == 1: the arg-max, lowest id on ties
    if (k != 1) {
        int c = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) c += v[j] > -INFINITY ? 1 : 0;
        int n_keep = sample_wave_sum_i(c);                            // finite logits
        if (k > 1 && k < EVO_SAMPLE_V) {
            const float kth = sample_unord((uint32_t)(keys[k - 1] >> 32));
            c = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) c += v[j] >= kth ? 1 : 0;     // ties with the k-th value stay
            n_keep = min(n_keep, sample_wave_sum_i(c));
        }
        const float T = temperature[s];
        const bool use_t = T != 1.0f && T > 0.f;
        // e = exp(logit - max) of the kept prefix, inclusive prefix sums P in position order
        float P[8];
        float run = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float d = use_t ? (v[j] - v0) / T : v[j] - v0;
            run += (lane * 8 + j < n_keep) ? expf(d) : 0.f;
            P[j] = run;
        }
        float scan = run;                                             // inclusive scan of the lane totals, fixed order
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const float up = __shfl_up(scan, d, 64);
            if (lane >= d) scan += up;
        }
        const float prev = __shfl_up(scan, 1, 64);
        const float base = lane == 0 ? 0.f : prev;                    // sum of every earlier lane's terms
#pragma unroll
        for (int j = 0; j < 8; ++j) P[j] += base;
        const float Z = __shfl(scan, 63, 64);
        const float p = top_p[s];
        if (p > 0.f && p < 1.f) {
            // the reference drops, in ASCENDING order, while the cumulative softmax is <= 1 - top_p: that cumulative value is the
            // suffix sum Z - (exclusive prefix) here
            const float thr = (1.0f - p) * Z;
            c = 0;
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float excl = j == 0 ? base : P[j - 1];
                c += (lane * 8 + j < n_keep && Z - excl > thr) ? 1 : 0;
            }
            n_keep = sample_wave_sum_i(c);
        }
        n_keep = max(n_keep, 1);
        float zk = 0.f;                                               // P at position n_keep - 1 (P never decreases)
#pragma unroll
        for (int j = 0; j < 8; ++j) zk = fmaxf(zk, lane * 8 + j < n_keep ? P[j] : 0.f);
        zk = wave_max(zk);
        const uint32_t r = philox4x32_10_x0((uint32_t)sid, (uint32_t)((uint64_t)sid >> 32), (uint32_t)cnt,
                                            (uint32_t)((uint64_t)cnt >> 32), seed_lo, seed_hi);
        const double u = ((double)(r >> 8) + 0.5) * 0x1p-24;
        const float target = (float)(u * (double)zk);
        c = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) c += (lane * 8 + j < n_keep && P[j] <= target) ? 1 : 0;
        pos = min(sample_wave_sum_i(c), n_keep - 1);                  // first position whose inclusive CDF exceeds u
    }
    const int tok = EVO_SAMPLE_V - 1 - (int)(uint32_t)keys[pos];      // 0 <= pos < 512, 0 <= tok < 512
    return SampleDraw{tok, raw[tok] - lse};
}

__global__ __launch_bounds__(64) void sample_rows_kernel(const void* __restrict__ logits, int logits_f32, int64_t ld,
                                                         const int32_t* __restrict__ top_k, const float* __restrict__ top_p,
                                                         const float* __restrict__ temperature, const uint8_t* __restrict__ allow,
                                                         uint32_t seed_lo, uint32_t seed_hi, const int64_t* __restrict__ stream_id,
                                                         int64_t* count, const uint8_t* __restrict__ active, int64_t* ids_out,
                                                         float* logprob_out, int64_t* hist_ids, float* hist_logits, int64_t hist_len) {
    __shared__ uint64_t keys[EVO_SAMPLE_V];
    __shared__ float raw[EVO_SAMPLE_V];
    const int64_t s = blockIdx.x;
    if (active && !active[s]) return;                                 // (the whole wave: before any barrier)
    const int64_t cnt = count ? count[s] : 0;
    const int64_t sid = stream_id ? stream_id[s] : s;
    const bool hist_ok = cnt >= 0 && cnt < hist_len;                  // (hist_len = 0 without history)
    const SampleDraw d = sample_draw_row(logits, logits_f32, ld, s, top_k, top_p, temperature, sample_allow_bits(allow), seed_lo, seed_hi, sid,
                                         cnt, (hist_logits && hist_ok) ? hist_logits + (s * hist_len + cnt) * EVO_SAMPLE_V : nullptr, keys, raw);
    if (threadIdx.x == 0) {
        ids_out[s] = d.tok;
        logprob_out[s] = d.logprob;
        if (hist_ids && hist_ok) hist_ids[s * hist_len + cnt] = d.tok;
        if (count) count[s] = cnt + 1;
    }
}

// The same draw with job control (specification: evo_amd/sh/sample.py finish_reason / sample_ctl): the row decides
// by itself that its job is over -- a stop token, an in-frame stop pattern at the end of its recorded tokens, or its own length limit --
// and clears its `active` byte, so the launches that follow skip it and the host learns of it from `length` whenever it cares to look.
// The patterns travel in the launch's arguments (at most 8 x 8 ids): no pattern memory on the device, fixed in a captured graph.
struct SampleStops {
    int32_t seq[EVO_SAMPLE_MAX_STOP_SEQ][EVO_SAMPLE_MAX_STOP_LEN];
    int32_t len[EVO_SAMPLE_MAX_STOP_SEQ];
    int32_t n_seq;
};

// Reasons 1 and 2 of the rule, by lane 0 once the row's token `tok` is recorded at cell `cnt` of its token history `h` (n = cnt + 1
// tokens): 1 the token is a stop token, 2 an in-frame stop pattern ends here, 0 neither.
__device__ __forceinline__ int sample_stop_reason(int tok, int64_t cnt, const uint8_t* __restrict__ stop_mask, const SampleStops& stops,
                                                  int64_t stop_frame, const int64_t* h) {
    const int64_t n = cnt + 1;
    if (stop_mask && ((stop_mask[tok >> 3] >> (tok & 7)) & 1u)) return 1;
    if (stops.n_seq > 0 && n % stop_frame == 0) {
        // the last `len` tokens against pattern q, newest first: the new token from its register, the others from the cells
        // cnt - 1 ... cnt - len + 1 >= 0 of this row, which earlier launches on this stream wrote; a pattern longer than n reads nothing
        for (int q = 0; q < stops.n_seq; ++q) {
            const int len = stops.len[q];
            if (len > n) continue;
            bool same = stops.seq[q][len - 1] == tok;
            for (int i = 1; i < len && same; ++i) same = h[cnt - i] == (int64_t)stops.seq[q][len - 1 - i];
            if (same) return 2;
        }
    }
    return 0;
}

__global__ __launch_bounds__(64) void sample_rows_ctl_kernel(const void* __restrict__ logits, int logits_f32, int64_t ld,
                                                             const int32_t* __restrict__ top_k, const float* __restrict__ top_p,
                                                             const float* __restrict__ temperature, const uint8_t* __restrict__ allow,
                                                             uint32_t seed_lo, uint32_t seed_hi, const int64_t* __restrict__ stream_id,
                                                             int64_t* count, uint8_t* active, int64_t* ids_out, float* logprob_out,
                                                             int64_t* hist_ids, float* hist_logits, float* hist_logprob, int64_t hist_len,
                                                             const int64_t* __restrict__ limit, const uint8_t* __restrict__ stop_mask,
                                                             const SampleStops stops, int64_t stop_frame, int64_t* length,
                                                             uint8_t* finish) {
    __shared__ uint64_t keys[EVO_SAMPLE_V];
    __shared__ float raw[EVO_SAMPLE_V];
    const int64_t s = blockIdx.x;
    if (!active[s]) return;                                           // (the whole wave: before any barrier)
    const int64_t cnt = count[s];
    const int64_t lim = limit[s];
    // nothing left to draw, or no cell left to record it in: the job ends here, by length, with no read of the logits or the history
    if (cnt < 0 || cnt >= lim || (hist_len > 0 && cnt >= hist_len)) {
        if (threadIdx.x == 0) {
            active[s] = 0;
            length[s] = cnt;
            finish[s] = 3;
        }
        return;
    }
    const int64_t sid = stream_id ? stream_id[s] : s;
    const SampleDraw d = sample_draw_row(logits, logits_f32, ld, s, top_k, top_p, temperature, sample_allow_bits(allow), seed_lo, seed_hi, sid,
                                         cnt, hist_logits ? hist_logits + (s * hist_len + cnt) * EVO_SAMPLE_V : nullptr, keys, raw);
    if (threadIdx.x == 0) {
        const int tok = d.tok;
        const int64_t n = cnt + 1;                                    // tokens recorded once this one is
        ids_out[s] = tok;
        logprob_out[s] = d.logprob;
        if (hist_ids) hist_ids[s * hist_len + cnt] = tok;             // (0 <= cnt < hist_len: checked above)
        if (hist_logprob) hist_logprob[s * hist_len + cnt] = d.logprob;
        count[s] = n;
        int reason = sample_stop_reason(tok, cnt, stop_mask, stops, stop_frame, hist_ids ? hist_ids + s * hist_len : nullptr);
        if (!reason && n >= lim) reason = 3;
        if (reason) {
            active[s] = 0;
            length[s] = n;
            finish[s] = (uint8_t)reason;
        }
    }
}

// The control kernel under a per-row token automaton (specification: evo_amd/sh/sample.py dfa_allowed / sample_dfa).
// Row s stands in row r = dfa_base[s] + dfa_state[s] of one table [n_states, 8]: column a is what drawing alphabet[a] does -- a next
// state (relative to the row's base), EVO_DFA_ACCEPT, or forbidden (any other negative value).  The permitted symbols, intersected with
// the global allow mask, are the lane's allow bits of the shared draw; lane 0 then moves the state.  The alphabet (at most 8 ids)
// travels in the launch's arguments like the stop patterns; the table row is one uniform 32-byte read in front of the sort.
struct SampleAlphabet {
    int32_t id[EVO_DFA_MAX_SYMBOLS];
    int32_t n_sym;
};

__global__ __launch_bounds__(64) void sample_rows_dfa_kernel(const void* __restrict__ logits, int logits_f32, int64_t ld,
                                                             const int32_t* __restrict__ top_k, const float* __restrict__ top_p,
                                                             const float* __restrict__ temperature, const uint8_t* __restrict__ allow,
                                                             uint32_t seed_lo, uint32_t seed_hi, const int64_t* __restrict__ stream_id,
                                                             int64_t* count, uint8_t* active, int64_t* ids_out, float* logprob_out,
                                                             int64_t* hist_ids, float* hist_logits, float* hist_logprob, int64_t hist_len,
                                                             const int64_t* __restrict__ limit, const uint8_t* __restrict__ stop_mask,
                                                             const SampleStops stops, int64_t stop_frame, int64_t* length,
                                                             uint8_t* finish, const SampleAlphabet alpha,
                                                             const int32_t* __restrict__ dfa_next, int64_t n_states,
                                                             const int64_t* __restrict__ dfa_base, int32_t* dfa_state) {
    __shared__ uint64_t keys[EVO_SAMPLE_V];
    __shared__ float raw[EVO_SAMPLE_V];
    const int64_t s = blockIdx.x;
    if (!active[s]) return;                                           // (the whole wave: before any barrier)
    const int64_t cnt = count[s];
    const int64_t lim = limit[s];
    if (cnt < 0 || cnt >= lim || (hist_len > 0 && cnt >= hist_len)) { // the control kernel's own check, unchanged
        if (threadIdx.x == 0) {
            active[s] = 0;
            length[s] = cnt;
            finish[s] = 3;
        }
        return;
    }
    const int lane = threadIdx.x;
    uint32_t abits = sample_allow_bits(allow);
    const int64_t base = dfa_base[s];
    const bool constrained = base >= 0;                               // (uniform over the wave, as everything up to the draw)
    int32_t nx[EVO_DFA_MAX_SYMBOLS];
#pragma unroll
    for (int a = 0; a < EVO_DFA_MAX_SYMBOLS; ++a) nx[a] = -1;
    if (constrained) {
        const int64_t q = dfa_state[s];
        const int64_t r = base + q;                                   // (base < 2^63 - 2^31 for any table that fits memory: no overflow)
        uint32_t dbits = 0;
        if (q >= 0 && r >= 0 && r < n_states) {
            const int4* row = (const int4*)(dfa_next + r * EVO_DFA_MAX_SYMBOLS);     // 16-byte aligned: the entry checks dfa_next
            const int4 lo = row[0], hi = row[1];
            nx[0] = lo.x; nx[1] = lo.y; nx[2] = lo.z; nx[3] = lo.w;
            nx[4] = hi.x; nx[5] = hi.y; nx[6] = hi.z; nx[7] = hi.w;
#pragma unroll
            for (int a = 0; a < EVO_DFA_MAX_SYMBOLS; ++a) {
                const int id = alpha.id[a];                           // 0 <= id < 512 for a < n_sym: the entry checks
                const bool ok = a < alpha.n_sym && (nx[a] >= 0 || nx[a] == EVO_DFA_ACCEPT);
                if (ok && (id >> 3) == lane) dbits |= 1u << (id & 7);
            }
        }
        abits &= dbits;
        if (sample_wave_sum_i(abits != 0 ? 1 : 0) == 0) {             // dead end: nothing is drawn, the state stays
            if (lane == 0) {
                active[s] = 0;
                length[s] = cnt;
                finish[s] = 5;
            }
            return;
        }
    }
    const int64_t sid = stream_id ? stream_id[s] : s;
    const SampleDraw d = sample_draw_row(logits, logits_f32, ld, s, top_k, top_p, temperature, abits, seed_lo, seed_hi, sid, cnt,
                                         hist_logits ? hist_logits + (s * hist_len + cnt) * EVO_SAMPLE_V : nullptr, keys, raw);
    if (lane == 0) {
        const int tok = d.tok;
        const int64_t n = cnt + 1;
        ids_out[s] = tok;
        logprob_out[s] = d.logprob;
        if (hist_ids) hist_ids[s * hist_len + cnt] = tok;             // (0 <= cnt < hist_len: checked above)
        if (hist_logprob) hist_logprob[s * hist_len + cnt] = d.logprob;
        count[s] = n;
        bool accepted = false;
        if (constrained) {
            int32_t nxt = -1;                                         // (the token is one of the permitted symbols: some a matches)
#pragma unroll
            for (int a = 0; a < EVO_DFA_MAX_SYMBOLS; ++a)
                if (a < alpha.n_sym && alpha.id[a] == tok) nxt = nx[a];
            if (nxt == EVO_DFA_ACCEPT) accepted = true;
            else dfa_state[s] = nxt;
        }
        int reason = sample_stop_reason(tok, cnt, stop_mask, stops, stop_frame, hist_ids ? hist_ids + s * hist_len : nullptr);
        if (!reason && accepted) reason = 4;
        if (!reason && n >= lim) reason = 3;
        if (reason) {
            active[s] = 0;
            length[s] = n;
            finish[s] = (uint8_t)reason;
        }
    }
}

extern "C" int evo_sample_rows_f32(const void* logits, int64_t logits_f32, int64_t ld, const int32_t* top_k, const float* top_p,
                                   const float* temperature, const void* allow, uint64_t seed, const int64_t* stream_id, int64_t* count,
                                   const uint8_t* active, int64_t* ids_out, float* logprob_out, int64_t* hist_ids, float* hist_logits,
                                   int64_t hist_len, int64_t S, int64_t V, void* stream) {
    if (!logits || !top_k || !top_p || !temperature || !ids_out || !logprob_out) return -1;
    if (S < 1 || S > 0x7fffffff || V != EVO_SAMPLE_V || ld < V || ld % 8 != 0) return -1;
    if (((uintptr_t)logits & 15) || ((uintptr_t)hist_logits & 15)) return -1;
    if ((hist_ids || hist_logits) && (!count || hist_len < 1)) return -1;
    if (!hist_ids && !hist_logits) hist_len = 0;
    hipLaunchKernelGGL(sample_rows_kernel, dim3((unsigned)S), dim3(64), 0, (hipStream_t)stream, logits, (int)(logits_f32 != 0), ld, top_k,
                       top_p, temperature, (const uint8_t*)allow, (uint32_t)seed, (uint32_t)(seed >> 32), stream_id, count, active,
                       ids_out, logprob_out, hist_ids, hist_logits, hist_len);
    return evo_launch_status();
}

// The stop rule of the control entries into the launch's arguments: -1 for what their contract refuses (stop_frame < 1, n_seq outside
// 0 ... 8, patterns without stop_seq / stop_seq_len / the token history they look back into, a pattern length outside 1 ... 8).
static int sample_pack_stops(SampleStops& stops, const int32_t* stop_seq, const int32_t* stop_seq_len, int64_t n_seq, int64_t stop_frame,
                             const int64_t* hist_ids) {
    if (stop_frame < 1 || n_seq < 0 || n_seq > EVO_SAMPLE_MAX_STOP_SEQ) return -1;
    if (n_seq > 0 && (!stop_seq || !stop_seq_len || !hist_ids)) return -1;
    for (int q = 0; q < EVO_SAMPLE_MAX_STOP_SEQ; ++q) {
        stops.len[q] = 0;
        for (int i = 0; i < EVO_SAMPLE_MAX_STOP_LEN; ++i) stops.seq[q][i] = -1;
    }
    stops.n_seq = (int32_t)n_seq;
    for (int q = 0; q < n_seq; ++q) {                                 // host arrays: read here, before the launch
        const int32_t len = stop_seq_len[q];
        if (len < 1 || len > EVO_SAMPLE_MAX_STOP_LEN) return -1;
        stops.len[q] = len;
        for (int i = 0; i < len; ++i) stops.seq[q][i] = stop_seq[q * EVO_SAMPLE_MAX_STOP_LEN + i];
    }
    return 0;
}

extern "C" int evo_sample_rows_ctl_f32(const void* logits, int64_t logits_f32, int64_t ld, const int32_t* top_k, const float* top_p,
                                       const float* temperature, const void* allow, uint64_t seed, const int64_t* stream_id, int64_t* count,
                                       uint8_t* active, int64_t* ids_out, float* logprob_out, int64_t* hist_ids, float* hist_logits,
                                       float* hist_logprob, int64_t hist_len, const int64_t* limit, const void* stop_mask,
                                       const int32_t* stop_seq, const int32_t* stop_seq_len, int64_t n_seq, int64_t stop_frame,
                                       int64_t* length, uint8_t* finish, int64_t S, int64_t V, void* stream) {
    if (!logits || !top_k || !top_p || !temperature || !ids_out || !logprob_out) return -1;
    if (!count || !active || !limit || !length || !finish) return -1;
    if (S < 1 || S > 0x7fffffff || V != EVO_SAMPLE_V || ld < V || ld % 8 != 0) return -1;
    if (((uintptr_t)logits & 15) || ((uintptr_t)hist_logits & 15)) return -1;
    const bool any_hist = hist_ids || hist_logits || hist_logprob;
    if (any_hist && hist_len < 1) return -1;
    if (!any_hist) hist_len = 0;
    SampleStops stops;
    if (sample_pack_stops(stops, stop_seq, stop_seq_len, n_seq, stop_frame, hist_ids) != 0) return -1;
    hipLaunchKernelGGL(sample_rows_ctl_kernel, dim3((unsigned)S), dim3(64), 0, (hipStream_t)stream, logits, (int)(logits_f32 != 0), ld,
                       top_k, top_p, temperature, (const uint8_t*)allow, (uint32_t)seed, (uint32_t)(seed >> 32), stream_id, count, active,
                       ids_out, logprob_out, hist_ids, hist_logits, hist_logprob, hist_len, limit, (const uint8_t*)stop_mask, stops,
                       stop_frame, length, finish);
    return evo_launch_status();
}

extern "C" int evo_sample_rows_dfa_f32(const void* logits, int64_t logits_f32, int64_t ld, const int32_t* top_k, const float* top_p,
                                       const float* temperature, const void* allow, uint64_t seed, const int64_t* stream_id, int64_t* count,
                                       uint8_t* active, int64_t* ids_out, float* logprob_out, int64_t* hist_ids, float* hist_logits,
                                       float* hist_logprob, int64_t hist_len, const int64_t* limit, const void* stop_mask,
                                       const int32_t* stop_seq, const int32_t* stop_seq_len, int64_t n_seq, int64_t stop_frame,
                                       int64_t* length, uint8_t* finish, const int32_t* dfa_alphabet, int64_t n_sym,
                                       const int32_t* dfa_next, int64_t n_states, const int64_t* dfa_base, int32_t* dfa_state, int64_t S,
                                       int64_t V, void* stream) {
    if (!logits || !top_k || !top_p || !temperature || !ids_out || !logprob_out) return -1;
    if (!count || !active || !limit || !length || !finish) return -1;
    if (!dfa_alphabet || !dfa_next || !dfa_base || !dfa_state) return -1;
    if (S < 1 || S > 0x7fffffff || V != EVO_SAMPLE_V || ld < V || ld % 8 != 0) return -1;
    if (((uintptr_t)logits & 15) || ((uintptr_t)hist_logits & 15) || ((uintptr_t)dfa_next & 15)) return -1;
    const bool any_hist = hist_ids || hist_logits || hist_logprob;
    if (any_hist && hist_len < 1) return -1;
    if (!any_hist) hist_len = 0;
    SampleStops stops;
    if (sample_pack_stops(stops, stop_seq, stop_seq_len, n_seq, stop_frame, hist_ids) != 0) return -1;
    if (n_sym < 1 || n_sym > EVO_DFA_MAX_SYMBOLS || n_states < 1 || n_states > EVO_DFA_MAX_STATES) return -1;
    SampleAlphabet alpha;
    alpha.n_sym = (int32_t)n_sym;
    for (int a = 0; a < EVO_DFA_MAX_SYMBOLS; ++a) alpha.id[a] = -1;
    for (int a = 0; a < n_sym; ++a) {                                 // a host array: read here, before the launch
        const int32_t id = dfa_alphabet[a];
        if (id < 0 || id >= EVO_SAMPLE_V) return -1;
        for (int b = 0; b < a; ++b)
            if (alpha.id[b] == id) return -1;
        alpha.id[a] = id;
    }
    hipLaunchKernelGGL(sample_rows_dfa_kernel, dim3((unsigned)S), dim3(64), 0, (hipStream_t)stream, logits, (int)(logits_f32 != 0), ld,
                       top_k, top_p, temperature, (const uint8_t*)allow, (uint32_t)seed, (uint32_t)(seed >> 32), stream_id, count, active,
                       ids_out, logprob_out, hist_ids, hist_logits, hist_logprob, hist_len, limit, (const uint8_t*)stop_mask, stops,
                       stop_frame, length, finish, alpha, dfa_next, n_states, dfa_base, dfa_state);
    return evo_launch_status();
}
