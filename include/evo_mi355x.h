/* evo_mi355x.h -- C ABI of libevo_mi355x.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * StripedHyena forward that evo-design/evo runs through `stripedhyena==0.2.2` + FlashAttention-2.
 *
 * The reference has no C FFI: its plugin surface is the Python API of `stripedhyena` as consumed by
 * `evo`.  Each entry point below replaces the vendor/third-party kernel(s) that the
 * reference reaches for one step of that forward; the reference-side call site that pins the step is
 * cited per function.  `evo_amd/ops.py` is the ctypes binding; INTEGRATION.md shows the stub a
 * maintainer of the reference would add.
 *
 * Conventions (every function):
 *   - raw DEVICE pointers (tensor.data_ptr()); bf16 = uint16 storage; "c64" = interleaved {re,im} f32;
 *   - `stream` is a hipStream_t passed as void* (torch.cuda.current_stream().cuda_stream);
 *   - no allocation, no host sync, no global state: safe to capture in a hipGraph; workspace is
 *     passed in by the caller; which kernel a call launches depends on its arguments alone (the library
 *     reads no environment variable);
 *   - return value is a hipError_t cast to int (0 = hipSuccess); -1 = bad argument.  The Python
 *     binding raises on non-zero;
 *   - alignment: every pointer to bf16 / f32 / c64 tensor data (activations, weights, states, tables, workspaces) is
 *     16-byte aligned unless a function says otherwise (the kernels load and store 16 bytes per lane), and NO MORE
 *     is ever needed: a row slice of a bf16 matrix whose rows are whole multiples of 16 bytes, one third of a
 *     packed qkv, a block of z^T are all legal operands.  Integer vectors (ids, target, pos / dyn_pos, ranges,
 *     mask, bad_flag) are read one element at a time and need only that element's own alignment -- the callers
 *     pass row slices of int64 id matrices; so do the per-row vectors of evo_sample_rows_f32 (see there).  The
 *     binding checks the addresses it passes (HipOps._check_address);
 *   - extents: a launch reads and writes nothing outside the extents its arguments describe -- no load and no
 *     store before the first or behind the last element of an operand (a ragged last tile is masked, not
 *     clamped into a neighbour), workspaces included; operands passed as const are never written.  Elements
 *     INSIDE an extent that a function calls pad / scratch / "may hold anything" may be read and, where the
 *     function says so, written.  tests/test_gpu_arena.py runs every entry point between poisoned guard bands.
 */
#ifndef EVO_MI355X_H
#define EVO_MI355X_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ABI version; bumped when a signature changes (the binding refuses a library whose version differs).
 *   2: evo_embed_bf16 gained `bad_flag`; evo_hyena_seg_state / evo_hyena_apply gained `mask`;
 *      evo_unembed_logprob_bf16 and evo_hyena_mfma added.
 *   3: evo_rope_append_decode_bf16 added; the fused decode launches take up to 8 rows at K = 4096.
 *   4: evo_hyena_mfma gained the carry-in state `s0`, the end state `s_out` and `poles`; evo_hyena_mfma_state added.
 *   5: evo_mlp_gate_mfma_bf16 (GELU * gate in the dense layer's epilogue), evo_linear_zg_mfma_bf16 (group-major result) and
 *      evo_hyena_mfma_zg (the single-pass operator on group-major z) added.
 *   6: evo_hyena_cs_zg (the single-pass operator with channel-stationary waves: outputs, end state or state-only walk; blocked y)
 *      and evo_linear_xblk_mfma_bf16 (the output projection on that blocked y) added.
 *   7: evo_hyena_ct (the same operator on channel-major z^T: no input window in LDS), evo_linear_t_mfma_bf16 (the projection with
 *      a transposed result) and evo_rmsnorm_rows_bf16 (RMSNorm with padded batch rows) added.
 *   8: evo_attn_fwd_causal_bf16 gained `vt_ws` (workspace for V^T: the round-5 prefill kernel of csrc/attn_w64.hip reads its V
 *      fragments from a transposed copy); evo_hyena_mfma, evo_hyena_mfma_state, evo_hyena_mfma_zg, evo_hyena_cs_zg and
 *      evo_linear_zg_mfma_bf16 REMOVED (the earlier forms of the single-pass Hyena operator and the group-major projection that
 *      fed them: every caller is on evo_hyena_ct).
 *   9: the RMSNorm passes folded into the dense layers around them: evo_linear_mfma_nf_bf16, evo_linear_xblk_mfma_nf_bf16,
 *      evo_mlp_gate_mfma_nf_bf16, evo_linear_t_mfma_nf_bf16 (the same launches with a per-row factor in / the rows' sums of squares
 *      out) and evo_rms_finalize_f32 added; no signature changed.
 *  10: evo_probe_copy_f4 and evo_probe_mfma_bf16 added (the box-calibration probes of bench.py's `box` block); evo_mlp_gate_small_m_bf16 and
 *      evo_norm_mlp_gate_small_m_bf16 gained `grouped` (the decode launches read l1 | l2 in the gated MFMA launch's row order: one weight set), evo_mlp_gate_small_m_bf16
 *      takes 5-64 rows on an MFMA form;
 *      evo_rope_qk_bf16 and evo_rope_append_decode_bf16 gained `q_scale`, evo_attn_fwd_causal_bf16 / evo_attn_decode_bf16 accept
 *      softmax_scale <= 0 = "queries pre-scaled" (the prefill attention kernel without its per-score multiply); evo_linear_small_m_bf16
 *      takes up to 64 rows and an optional workspace (`ws`, `ws_bytes`: split over K across workgroups for the narrow layers); evo_hyena_ct gained `y_row_pitch` (rows of y between two batch rows: the scoring path runs the 512 k main tokens
 *      of every row through the operator and the one token behind them through the single-token launch, see below).
 *  11: evo_pool_rows_bf16 added (sequence embeddings: masked row pooling with the final RMSNorm optionally fused in); no signature changed.
 *  12: evo_sample_rows_f32 added (seeded sampling on the device); no signature changed.
 *  13: evo_unembed_profile_bf16 added (the fused scoring tail with the log-probs of up to 8 chosen vocabulary ids per row); no signature changed.
 *  14: evo_attn_fwd_prefix_bf16 and evo_attn_prefix_vt_bf16 added (causal attention whose keys are ONE prefix shared by every batch row plus
 *      each row's own suffix: variant scoring from a cached reference); no signature changed.
 *  15: evo_attn_decode_prefix_bf16 (decode attention of rows that continue SHARED stored prompts: the copies of a prompt in a decode pool
 *      read one K/V of it) and evo_rope_append_decode_at_bf16 (the decode rotary + append with the cache row given apart from the
 *      position) added; no signature changed.
 *  16: evo_hyena_state_at_zt added (the Hyena end state and FIR history at every row's OWN last token: ragged batched prefill); no
 *      signature changed.
 *  17: evo_sample_rows_ctl_f32 added (the seeded sampler with job control: stop tokens, in-frame stop patterns and per-row length
 *      limits decided on the device); no signature changed.
 *  18: evo_sample_rows_dfa_f32 added (the control sampler under a per-row token automaton: constrained generation); no signature
 *      changed.
 *  19: evo_kv_quant_fp8, evo_rope_append_decode_fp8 and evo_attn_decode_fp8 added (an opt-in FP8 e4m3fn KV cache for decode: the
 *      quantising stores and the decode attention that reads them, csrc/kv_fp8.hip); no signature changed.
 *  20: evo_w_quant_fp8, evo_linear_small_m_w8, evo_norm_linear_small_m_w8, evo_hyena_decode_fused_small_m_w8, evo_mlp_gate_small_m_w8
 *      and evo_norm_mlp_gate_small_m_w8 added (opt-in FP8 e4m3fn WEIGHTS for the decode step at 1-8 rows, csrc/gemv_fp8.hip); no
 *      signature changed.
 *      Added since under ABI 20, no signature changed: the paged KV entries, the beam search entries, and evo_linear_rowinv_bf16 /
 *      evo_mlp_gate_rowinv_bf16 (the row-invariant dense launches of the decode pool's opt-in batch-invariant step, csrc/gemv_inv.hip).
 *      evo_repeat_rows_f32 (k-mer repeat control in front of the decode pool's sampler launch, csrc/repeat.hip).
 *      evo_linear_skinny_w8 / evo_mlp_gate_skinny_w8 (FP8 weights at 5-64 rows on the MFMA weight-streaming forms, csrc/skinny_fp8.hip).
 *      A binding that needs them finds out at load time: every entry it declares must be exported. */
#define EVO_ABI_VERSION 20
int evo_abi_version(void);

/* ---- embedding gather ------------------------------------------------------------------------
 * replaces VocabParallelEmbedding.embed (ATen gather)    [REF evo/scoring.py:81; evo/models.py:136]
 * ids [n_tok] int64, weight [vocab, D] bf16 -> out [n_tok, D] bf16.  An id outside [0, vocab) never
 * indexes the table: its output row is zeros and *bad_flag (device int, may be NULL; the caller zeroes
 * it) is set to 1 -- the binding raises IndexError where F.embedding would device-assert. */
int evo_embed_bf16(const int64_t* ids, const void* weight, void* out,
                   int64_t n_tok, int64_t D, int64_t vocab, int* bad_flag, void* stream);

/* ---- RMSNorm -----------------------------------------------------------------------------------
 * replaces the eager RMSNorm chain (norm, div, mul)      [REF evo/configs/evo-1-8k-base_inference.yml:13,31]
 *   out = scale * x / (||x||_2 * D^-1/2 + eps)            (eps OUTSIDE the root)
 * x [M, D] bf16 -> out [M, D] bf16, fp32 accumulation, single output rounding.
 * If `bias` != NULL the row is first updated in place, x <- bf16(x + bias), and the norm is taken of
 * the updated row (this folds the out_proj / out_filter_dense bias add and the residual write). */
int evo_rmsnorm_bf16(void* x, const void* bias, const void* scale, void* out,
                     int64_t M, int64_t D, float eps, void* stream);

/* ---- Hyena operator, parallel (prefill / scoring) form ------------------------------------------
 * replaces HyenaInferenceEngine.parallel_fir + ParallelHyenaFilter.compute_filter + parallel_iir
 * (+ prefill_via_modal_fft)                               [REF evo/configs/evo-1-8k-base_inference.yml:8,10,14,33,37;
 *                                                          evo/generation.py:111-114]
 * Three launches over a (batch, head, time-segment) decomposition; the long convolution
 *   y_t = sum_{j<=t} h_{t-j} x1v_j,  h_k = Re sum_s R_s p_s^k
 * is evaluated EXACTLY through its 8 complex modes (S_t = p S_{t-1} + x1v_t; y_t = Re sum R_s S_t),
 * so no filter and no FFT buffer ever touches HBM.
 *
 *   z        [B, T, 3*D] bf16   projections output, channel-last; channel c = h*3*hd + g*hd + j,
 *                               g in {0:x2, 1:x1, 2:v}  (column split, hd = D / n_heads = 128)
 *   z_halo   [B, 2, 3*D] bf16 or NULL: rows t=-2,-1 (sequence-parallel halo; NULL = zeros)
 *   fir_w    [3*D, 3] bf16      short_filter_weight (cross-correlation taps; tap 2 hits z_t)
 *   fir_b    [3*D]    bf16      short_filter_bias
 *   poles, residues [D, 8, 2] f32
 *   dskip    [D] bf16           filter.D
 *   seg_len                     time-segment length C (multiple of 4); n_seg = ceil(T / C)
 *   agg      [B, n_seg, D, 8] c64 workspace:  (1) seg_state writes each segment's end state from a
 *                               zero start; (2) carry_scan rewrites it in place into the state ENTERING
 *                               each segment; (3) apply reads it.
 *   s0       [B, D, 8] c64 or NULL: state entering t=0 (sequence-parallel carry-in / resumed prefill)
 *   s_final  [B, D, 8] c64 or NULL: state after t=T-1  (== upstream prefill_via_modal_fft)
 *   y        [B, T, D] bf16     (y_conv + x1v * dskip) * x2, channel-last
 *   mask     [B, T] uint8 or NULL: upstream's `padding_mask` (1 = token, 0 = pad): the FIR output (x2, x1, v) of
 *                               a padded position is zero, as engine.parallel_fir multiplies it.  evo never passes one.
 */
int evo_hyena_seg_state(const void* z, const void* z_halo, const void* fir_w, const void* fir_b,
                        const float* poles, float* agg, const uint8_t* mask,
                        int64_t B, int64_t T, int64_t D, int64_t n_heads, int64_t seg_len, void* stream);
int evo_hyena_carry_scan(float* agg, const float* poles, const float* s0, float* s_final,
                         int64_t B, int64_t T, int64_t D, int64_t seg_len, void* stream);
/* sequence-parallel fix-up (new; the reference has no multi-GPU path): `agg` already scanned with a zero
 * carry-in gets p^(k*seg_len) * s0 added to segment k once the state s0 entering this shard is known. */
int evo_hyena_carry_add(float* agg, const float* poles, const float* s0,
                        int64_t B, int64_t T, int64_t D, int64_t seg_len, void* stream);
int evo_hyena_apply(const void* z, const void* z_halo, const void* fir_w, const void* fir_b,
                    const float* poles, const float* residues, const void* dskip,
                    const float* agg, void* y, const uint8_t* mask,
                    int64_t B, int64_t T, int64_t D, int64_t n_heads, int64_t seg_len, void* stream);

/* ---- Hyena operator, single-pass matrix-core form (scoring, cached prefill, sequence-parallel shards) -------
 * replaces the same reference functions as the three launches above (parallel_fir + compute_filter +
 * parallel_iir, and prefill_via_modal_fft for `s_out`)     [REF evo/configs/evo-1-8k-base_inference.yml:8,10,14,33,37;
 *                                                            evo/generation.py:111-117,152 for the cached form]
 * One launch, z read once, y written once (csrc/hyena_ct.hip; rounds 2-4 shipped three earlier forms of it -- token-major,
 * group-major with channel-stationary waves -- which round 5 retired: this is the only single-pass kernel).  A wave owns two
 * channels for a 512-step tile: its lanes' FIR outputs ARE the B operands of the block-Toeplitz MFMAs
 * (v_mfma_f32_16x16x32_bf16, operands split into bf16 hi + lo terms, fp32 accumulation), the 16 blocks' modal states meet in a
 * DPP scan in fp32, the carry product runs on the matrix cores with hi/lo-split states.
 *   zt     CHANNEL-MAJOR z: [zt_pitch / 256][3 D][256] bf16, the projection's result TRANSPOSED and stored in blocks of 256
 *          positions -- column c = h*3*hd + g*hd + j of z (the reference's order, no regrouping), position p at element
 *          ((p / 256) * 3 D + c) * 256 + p % 256; written by evo_linear_t_mfma_bf16.  Batch row b, token t sits at position
 *          zt_row0 + b * row_pitch + t.  A lane's eight steps of one channel are 16 consecutive bytes, loaded straight into the
 *          registers the FIR reads: no window in LDS, no DMA, no bank conflicts.  row_pitch % 8 == 0, zt_row0 % 8 == 0,
 *          zt_pitch % 256 == 0, zt_pitch * 3 D * 2 < 4 GiB, zt 16-byte aligned; positions between T and row_pitch may hold anything.
 *   tail_T != 0 (the "tail form", T = 512 k + r with r <= 8: tail_T = 512 k): tokens t >= tail_T of batch row b sit at position
 *          tail_pos0 + 8 b + (t - tail_T) instead (a tail block behind the main area, filled by the weight-streaming dense layer:
 *          rows of 512 k positions need no padding and the projection no extra round of tiles; evo_amd/ops.py zt_layout).
 *   z_halo [B, 2, 3 D] bf16 in the reference's column order (rows = steps -2, -1) or NULL
 *   table  [D, 52, 64] u32: per-channel MFMA operand constants (evo_amd/hyena_tables.py mfma_operand_table; filter.D folded into
 *          the block-Toeplitz diagonal)
 *   s0     [B, D, 8] c64 or NULL: modal state entering t = 0 (resumed prefill / sequence-parallel carry-in)
 *   s_out  [B, D, 8] c64 or NULL: state after t = T-1; needs `poles` [D, 8] c64 (fp32 pairs).  T % 512 == 0: the carry of the last tile, stored
 *          from registers; otherwise the last block's steps are walked from the state entering it (fp32 recurrence, ~half a tile's time per row)
 *   state_only != 0: no y (may be NULL), only s_out -- stage 1 of a sequence-parallel shard, whose end state from a zero carry-in
 *          goes to the other ranks before anybody can finish its outputs (new; the reference has no multi-GPU path)
 *   y      [B, T, D] bf16, or with y_blocked_rows != 0 BLOCKED: [ceil(y_blocked_rows / 128)][D / 16][128][16] bf16 -- the
 *          [y_blocked_rows, D] matrix with a group's 16 channels of 128 consecutive rows kept together (whole cache lines per
 *          store; evo_linear_xblk_mfma_bf16 reads it); batch row b, token t is row y_row0 + b y_row_pitch + t of that matrix (y_row0 > 0:
 *          the row groups of a sequence-parallel shard write into one tensor)
 *   y_row_pitch (ABI 10): rows of y between two batch rows, 0 = T.  > T: the caller owns rows T .. y_row_pitch - 1 behind every batch
 *          row (T = 512 k + 1 scoring batches: the operator walks the 512 k tokens in whole tiles and returns s_out, the last token of every
 *          row is one evo_hyena_decode_fused_small_m step from that state -- a ragged tile with ONE valid step costs a full tile's issue
 *          time, 8 of 136 tile steps at 8 x 8,193)
 *   no mask (padding_mask shapes take the three-launch form).  D == n_heads * 128. */
int evo_hyena_ct(const void* zt, const void* z_halo, const void* fir_w, const void* fir_b, const void* table, void* y,
                 const float* s0, float* s_out, const float* poles, int64_t B, int64_t T, int64_t D, int64_t n_heads,
                 int64_t zt_pitch, int64_t row_pitch, int64_t zt_row0, int64_t tail_T, int64_t tail_pos0, int64_t state_only,
                 int64_t y_blocked_rows, int64_t y_row0, int64_t y_row_pitch, void* stream);

/* ---- Hyena end state of a ragged batch: the state and FIR history at every row's OWN last token ----------------------------
 * what a cached prefill hands to decode (`s_out` of evo_hyena_ct, the last two rows of z), per row    [REF evo/generation.py:111-117,152]
 * for a batch of right-padded prompts of unequal length run through ONE forward (csrc/hyena_ragged.hip).  The state at T cannot be
 * rolled back to lens[b] < T (that divides by p^(T - lens[b]), |p| < 1), so it is computed from z^T directly: time is cut into
 * segments of EVO_HYENA_RAGGED_SEG steps, a thread walks (row, segment, channel) from a zero state with the per-step fp32 arithmetic of
 * evo_hyena_seg_state, segments wholly behind lens[b] exit at once, and a second small launch combines a row's segments with p^n in
 * fp64 (as evo_hyena_carry_scan does).  Two launches whatever B and the lengths are; lens is read on the device only.
 *   zt      the tensor evo_hyena_ct reads, plain form only (no tail block): batch row b, token t at position zt_row0 + b * row_pitch + t
 *   lens    [B] int64, DEVICE memory; a value outside [1, T] is clamped into it
 *   s_out   [B, D, 8] c64: the state after step lens[b] - 1 from a zero start (no carry-in, no halo: a ragged batch starts at t = 0)
 *   fir_out [B, 3 D, 2] bf16: z[b, lens[b] - 2], z[b, lens[b] - 1] of every column in the reference's order, oldest first, zeros where
 *           t < 0 -- the bits of zt, untouched
 *   ws      workspace of ws_bytes bytes, 16-byte aligned; ws == NULL: nothing is launched and the bytes needed are returned
 * Positions t >= lens[b] of a row and pad positions of the layout may hold anything (NaN included): nothing there reaches an output.
 * Returns -1 before any launch unless D == n_heads * 128, T % 64 == 0 || B == 1, row_pitch % 8 == 0 (>= T for B > 1), zt_row0 % 8 == 0,
 * zt_pitch % 256 == 0, the rows fit zt_pitch, every pointer but ws is non-null, and ws_bytes covers the need. */
#define EVO_HYENA_RAGGED_SEG 256
int evo_hyena_state_at_zt(const void* zt, const int64_t* lens, const void* fir_w, const void* fir_b, const float* poles,
                          float* s_out, void* fir_out, float* ws, int64_t ws_bytes,
                          int64_t B, int64_t T, int64_t D, int64_t n_heads,
                          int64_t zt_pitch, int64_t row_pitch, int64_t zt_row0, void* stream);

/* The Hyena block's output projection on the blocked y of evo_hyena_ct               [REF stripedhyena/model.py ParallelGatedConvBlock:
 * out_filter_dense]:  y [M, N] = x . w^T (+ bias [N]) (+ residual [M, N], may alias y), x = [M / 128][K / 16][128][16] bf16.  The persistent dense
 * layer of evo_linear_mfma_bf16 with other source addresses for its X tiles; M % 256 == 0, N % 256 == 0, K % 64 == 0, K >= 128. */
int evo_linear_xblk_mfma_bf16(const void* x_blk, const void* w, const void* bias, const void* residual, void* y,
                              int64_t M, int64_t N, int64_t K, void* stream);

/* The Hyena projection with a transposed result              [REF stripedhyena/model.py ParallelGatedConvBlock.forward: projections]:
 * zt [Mp / 256][N][256] bf16 = (x [Mp, K] . w [N, K]^T + bias [N])^T in blocks of 256 positions (an output tile of the kernel = one
 * contiguous 128 KiB piece) -- the persistent dense layer of evo_linear_mfma_bf16 launched with its operands swapped (rows of the
 * result = output features, columns = tokens; the bias runs along the rows; the tile raster mirrored), bit-identical to that
 * layer's result, transposed.  Mp % 256 == 0 (the caller pads x: see evo_rmsnorm_rows_bf16), N % 256 == 0, K % 64 == 0, K >= 128. */
int evo_linear_t_mfma_bf16(const void* x, const void* w, const void* bias, void* zt, int64_t Mp, int64_t N, int64_t K, void* stream);

/* evo_rmsnorm_bf16 with the output rows in the order of a channel-major z^T: token t < Tm of batch row b (row b * T + t of x [M = B T, D])
 * -> row b * Tp + t of out (Tp >= Tm; the pad rows are not written), the last T - Tm tokens of a row -> the compact tail rows
 * tail0 + b * (T - Tm) + (t - Tm).  Tm = T: no tail.  Same arithmetic, same bits per row. */
int evo_rmsnorm_rows_bf16(void* x, const void* bias, const void* scale, void* out, int64_t M, int64_t D, float eps,
                          int64_t T, int64_t Tp, int64_t Tm, int64_t tail0, void* stream);

/* ---- Hyena operator, recurrent (decode) form -----------------------------------------------------
 * replaces step_fir + step_iir                             [REF evo/generation.py:111-114,138-155]
 *   z_t [B, 3D] bf16; fir_state [B, 3D, 2] bf16 (in/out, oldest first); iir_state [B, D, 8] c64 (in/out)
 *   y [B, D] bf16 */
int evo_hyena_step(const void* z_t, void* fir_state, float* iir_state,
                   const void* fir_w, const void* fir_b, const float* poles, const float* residues,
                   const void* dskip, void* y, int64_t B, int64_t D, int64_t n_heads, void* stream);

/* ---- rotary embedding -----------------------------------------------------------------------------
 * replaces flash_attn's Triton rotary kernel               [REF evo/configs/evo-1-131k-base_inference.yml:39-40]
 * NeoX (non-interleaved) pairs (i, i+hd/2), in place on the q and k thirds of a packed
 * qkv [B, T, 3, H, hd] bf16.  cos/sin [T, hd/2] f32 are host-built for absolute positions
 * pos0..pos0+T-1 (already divided by the interpolation factor, already rounded to bf16 values).
 * q_scale (ABI 10; > 0): the rotated QUERY rows are multiplied by it before their one rounding -- the caller passes
 * softmax_scale * log2(e) and then calls evo_attn_fwd_causal_bf16 / evo_attn_decode_bf16 with softmax_scale = 0 ("queries pre-scaled":
 * a score is an exponent, the prefill kernel's per-score multiply disappears); 1.0 = plain rotary (exact: the bits of ABI 9). */
int evo_rope_qk_bf16(void* qkv, const float* cos_t, const float* sin_t,
                     int64_t B, int64_t T, int64_t H, int64_t hd, float q_scale, void* stream);

/* decode form: rotary on the q and k rows of ONE token per stream, each at its own position, and the append of (k, v) to
 * the KV cache, in one launch                                  [REF evo/generation.py:138-155; flash_attn_with_kvcache's
 *                                                              rotary + cache-update arguments]
 *   qkv [B, 3, H, hd] bf16 contiguous (q and k rotated in place); kv = the cache [.., cap, 2, H, hd] bf16 with element strides
 *   (batch, token, k|v, head), each a multiple of 8; pos [B] device int64: row b is written at token pos[b] (< cap: the caller's
 *   bound); inv_freq [hd/2] f32; angle = (pos / scaling) * inv_freq, cos / sin rounded to bf16 values as the cached tables are.
 *   Bit-identical to evo_rope_qk_bf16 with a table for those positions followed by the indexed copy. */
int evo_rope_append_decode_bf16(void* qkv, void* kv, const int64_t* pos, const float* inv_freq, float scaling,
                                int64_t B, int64_t H, int64_t hd, int64_t kv_sb, int64_t kv_st, int64_t kv_sw, int64_t kv_sh,
                                float q_scale, void* stream);
/* the same (ABI 15) with the cache row given apart from the position: the angle comes from pos[b] (absolute), the row is written at
 * token widx[b] of the cache (device int64 [B], < cap) -- a slot whose own cache starts behind a prompt stored elsewhere
 * (evo_attn_decode_prefix_bf16).  widx == pos is evo_rope_append_decode_bf16 bit for bit (one kernel serves both). */
int evo_rope_append_decode_at_bf16(void* qkv, void* kv, const int64_t* pos, const float* inv_freq, float scaling,
                                   int64_t B, int64_t H, int64_t hd, int64_t kv_sb, int64_t kv_st, int64_t kv_sw, int64_t kv_sh,
                                   float q_scale, const int64_t* widx, void* stream);

/* ---- causal multi-head attention forward ------------------------------------------------------------
 * replaces flash_attn_2_cuda fwd / flash_attn_with_kvcache  [REF README.md:47-50; evo/configs/evo-1-8k-base_inference.yml:9,30]
 * MFMA 32x32x16 bf16 tiles, online softmax in fp32, head dim 128 only.
 *   q [B, Tq, H, 128], k/v [B, Tk, H, 128] bf16 with explicit element strides (batch, token, head);
 *   o [B, Tq, H, 128] bf16 contiguous.  Query i may see key j iff j <= i + q_pos0 (q_pos0 = absolute
 *   position of query 0 minus absolute position of key 0).
 *   vt_ws: caller-owned workspace of B * H * 128 * (Tk rounded up to 64) bf16, or NULL.  Query ranges longer than 128 rows run
 *   the 64-rows-per-wave kernel (csrc/attn_w64.hip: one wave per SIMD, K / V tiles through LDS-DMA rings), which reads V^T:
 *   a pre-pass launch writes it into vt_ws.  With vt_ws == NULL (or Tq <= 128) the kernels of rounds 1-4 run (csrc/attn.hip).
 *   softmax_scale <= 0 (ABI 10): the queries carry softmax_scale * log2(e) already (evo_rope_qk_bf16's q_scale) -- scores are taken as
 *   exponents in the log2 domain; same for evo_attn_decode_bf16. */
int evo_attn_fwd_causal_bf16(const void* q, const void* k, const void* v, void* o,
                             int64_t B, int64_t H, int64_t Tq, int64_t Tk, int64_t q_pos0,
                             int64_t q_sb, int64_t q_st, int64_t q_sh,
                             int64_t k_sb, int64_t k_st, int64_t k_sh,
                             int64_t v_sb, int64_t v_st, int64_t v_sh,
                             float softmax_scale, void* vt_ws, void* stream);

/* shared prefix + private suffix (ABI 14): B rows that continue ONE common prefix -- the variants of a reference sequence, scored from
 * the reference's KV cache -- without B copies of the prefix's K, V and V^T.  (No counterpart in the reference, which forwards every
 * variant whole [REF evo/scoring.py:80-84].)
 *   q [B, Tq, H, 128]; k / v [B, Tq, H, 128]: the rows' OWN keys (the suffix), strided like above (e.g. the thirds of a packed qkv);
 *   k_pre [P, H, 128]: the prefix keys, NO batch dimension, element strides (token kp_st, head kp_sh) -- a view into a KV cache
 *   [1, cap, 2, H, 128] works without a copy; o [B, Tq, H, 128] bf16 contiguous.
 *   Query i of row b sees prefix keys 0 .. P-1 and suffix keys 0 .. i of row b: the result is bit for bit that of
 *   evo_attn_fwd_causal_bf16 (with vt_ws) on k = cat(k_pre, k_b), Tk = P + Tq, q_pos0 = P -- same key tiles, same order, same arithmetic
 *   (csrc/attn_w64.hip SEG: a 64-key tile lies in one segment; its descriptors pick the segment with scalar selects).
 *   Contract: P >= 64, P % 64 == 0 and Tq >= 129, otherwise -1 without a launch: only the 64-rows-per-wave form is built; shorter
 *   ranges are the caller's business (evo_amd/scoring.py plans variant suffixes accordingly).
 *   V^T workspaces (keys contiguous, bf16):
 *     vt_pre  the PREFIX plane [H][128][vtp_row], vtp_row % 64 == 0, vtp_row >= P, 128 * vtp_row * 2 < 4 GiB: written ONCE per reference
 *             and layer by evo_attn_prefix_vt_bf16 below (for as many keys as any later call uses as its prefix: a call with a shorter P
 *             reads the first P columns of the same plane), never by this entry -- const here;
 *     vt_ws   the SUFFIX planes [B][H][128][Tq rounded up to 64], written by this entry's pre-pass on every call.
 *   softmax_scale <= 0: the queries are pre-scaled, as above. */
int evo_attn_fwd_prefix_bf16(const void* q, const void* k, const void* v, const void* k_pre, const void* vt_pre, void* o,
                             int64_t B, int64_t H, int64_t Tq, int64_t P,
                             int64_t q_sb, int64_t q_st, int64_t q_sh,
                             int64_t k_sb, int64_t k_st, int64_t k_sh,
                             int64_t v_sb, int64_t v_st, int64_t v_sh,
                             int64_t kp_st, int64_t kp_sh, int64_t vtp_row,
                             float softmax_scale, void* vt_ws, void* stream);
/* v_pre [P, H, 128] (element strides vp_st, vp_sh; no batch dimension) -> vt_pre [H][128][vt_row]: columns 0 .. P-1 hold V^T, the
 * columns up to the next multiple of 64 zeros, later ones are not written.  vt_row % 64 == 0, vt_row >= P, P >= 1. */
int evo_attn_prefix_vt_bf16(const void* v_pre, void* vt_pre, int64_t P, int64_t H, int64_t vp_st, int64_t vp_sh, int64_t vt_row,
                            void* stream);

/* decode form (one query per sequence, Tq = 1): split-K over the key range ("flash-decoding") + combine.
 * replaces flash_attn_with_kvcache                           [REF evo/generation.py:109-110,138-155]
 *   q [B, 1, H, 128] (q_sb, q_sh strides), k/v views of the KV cache [B, cap, H, 128];
 *   dyn_pos: NULL -> the query sits at position Tk-1 and sees keys [0, Tk);  non-NULL -> device int64 [B]:
 *            row b's query sits at p_b = dyn_pos[b] and sees keys [0, p_b] (Tk is then only the cache capacity
 *            bound).  The launch no longer depends on the positions, so a captured hipGraph can be replayed for
 *            every token, and rows may be at DIFFERENT positions (continuous batching of decode streams);
 *   part_o [B, H, n_splits, 128] f32 and part_ml [B, H, n_splits, 2] f32: caller-owned workspace;
 *   n_splits <= 1024.  A bandwidth kernel (the KV cache is read once, 512 * H bytes per key): a WAVE owns a split = every
 *   n_splits-th 64-key block, requests the 32 KiB of a block at once and needs neither LDS nor barriers.
 *   That kernel (attn_decode_stream_kernel) addresses a key by a 32-bit byte offset from the (batch, head) base, so it runs while
 *   Tk * k_st * 2 < 2^32 - 1 and Tk * v_st * 2 < 2^32 - 1 (Tk as passed: the capacity).  A cache view beyond that -- e.g. capacity
 *   262,144 at H = 32: 4 GiB per batch row -- takes the SECOND kernel, attn_fwd_kernel<true> (csrc/attn.hip: the MFMA split kernel,
 *   64-bit tile bases, split s = ceil(n_tiles / n_splits) CONSECUTIVE 64-key tiles, splits past the last tile leave (m, l) = (-inf, 0)),
 *   with the same part_o / part_ml layout, the same combine launch and the same bounds (tests/PARITY.md row 22g). */
int evo_attn_decode_bf16(const void* q, const void* k, const void* v, void* o,
                         int64_t B, int64_t H, int64_t Tk,
                         int64_t q_sb, int64_t q_sh,
                         int64_t k_sb, int64_t k_st, int64_t k_sh,
                         int64_t v_sb, int64_t v_st, int64_t v_sh,
                         const int64_t* dyn_pos, float* part_o, float* part_ml, int64_t n_splits,
                         float softmax_scale, void* stream);

/* ---- FP8 (OCP e4m3fn) KV cache for decode (ABI 19; csrc/kv_fp8.hip) ----------------------------------------------------
 * The three entries below stand where the reference calls flash_attn_with_kvcache  [REF evo/generation.py:138-155]; the reference has
 * no quantised cache.  gfx950's FP8 is OCP e4m3fn (max 448, no infinities), not MI300's fnuz.
 *   THE RULE.  A cached row is the 128 values of one (stream b, token t, K-or-V, head h).  With a = max |x_j| over the row, e is the
 *   smallest integer with a * 2^-e <= 448, clamped to [-126, 120]; a = 0 gives e = 0.  Stored: 128 bytes RNE_e4m3fn(x_j * 2^-e) and one
 *   f32 scale 2^e.  The product is exact and at most 448 in magnitude (one rounding, never saturated); byte * scale is exact in fp32.
 *   In torch: (x.float() * 2.0 ** -e).to(torch.float8_e4m3fn).  Inputs are finite; NaN / Inf rows are unspecified.
 *   THE CACHE OPERAND of a layer (the same seven strides in all three entries):
 *     kv_data  [B, cap, 2, H, 128] bytes, BYTE strides d_sb (batch), d_st (token), d_sw (K | V), d_sh (head), each a multiple of 16
 *              (d_st, d_sw, d_sh >= 128), 16-byte aligned;
 *     kv_scale [B, 2, H, cap] f32, ELEMENT strides s_sb (batch), s_sw (K | V), s_sh (head); tokens are contiguous, so the 64 scales of
 *              a key block are one 256-byte run for the wave that streams that head.
 *   8,448 bytes per key and layer at H = 32 instead of 16,384.
 *   All three return -1 without a launch on a null pointer, a misaligned pointer (16 bytes for data, 8 for pos / dyn_pos, 4 for f32
 *   vectors), a stride that breaks the rules above, or a size <= 0.
 *
 * evo_kv_quant_fp8: rows [B, T, H, 128] bf16 of K and of V (strided views with element strides batch / token / head, each a multiple
 * of 8: the two thirds of a packed qkv) -> cache tokens t0 .. t0 + T - 1 of every batch row, by the rule.  t0 + T <= cap or -1.  Serves
 * the cached prefill at any T (ragged batches included) and the scalar-offset single-token step (rotary first, evo_rope_qk_bf16).
 * Nothing outside those tokens is written. */
int evo_kv_quant_fp8(const void* k, const void* v, void* kv_data, float* kv_scale,
                     int64_t B, int64_t T, int64_t H, int64_t t0, int64_t cap,
                     int64_t k_sb, int64_t k_st, int64_t k_sh, int64_t v_sb, int64_t v_st, int64_t v_sh,
                     int64_t d_sb, int64_t d_st, int64_t d_sw, int64_t d_sh, int64_t s_sb, int64_t s_sw, int64_t s_sh,
                     void* stream);
/* evo_rope_append_decode_bf16 with the append quantised: rotary on q and k of qkv [B, 3, H, 128] in place at pos[b] -- the bits left in
 * qkv are exactly that entry's, q_scale included -- then k (rotated) and v go to token pos[b] of the FP8 cache by the rule.  One
 * launch, per-row device positions (< cap: the caller's bound), capturable.  hd must be 128.  There is no `widx` form: a prompt store
 * stays bf16. */
int evo_rope_append_decode_fp8(void* qkv, void* kv_data, float* kv_scale, const int64_t* pos, const float* inv_freq, float scaling,
                               int64_t B, int64_t H, int64_t hd,
                               int64_t d_sb, int64_t d_st, int64_t d_sw, int64_t d_sh, int64_t s_sb, int64_t s_sw, int64_t s_sh,
                               float q_scale, void* stream);
/* evo_attn_decode_bf16's contract on an FP8 cache: q [B, 1, H, 128] bf16 (q_sb, q_sh element strides), o [B, 1, H, 128] bf16
 * contiguous, Tk = the keys (dyn_pos NULL) or the capacity bound (dyn_pos [B] device int64: row b sees keys [0, dyn_pos[b]]; nothing
 * behind a row's position is read), the same part_o / part_ml workspace, the same split partition (split s takes the 64-key blocks s,
 * s + n_splits, ...) and the same combine launch.  softmax_scale <= 0: pre-scaled queries.  The kernel (attn_decode_fp8_kernel) is the
 * streaming form: a wave owns a split and keeps two 32-key halves (8 KiB each: 4 KiB K, 4 KiB V, 256 B of scales) in flight while it
 * reduces a third; a key's scale multiplies its fp32 score once, a V row's scale its probability once.  It addresses keys with 32-bit
 * byte offsets and has no second form: Tk * d_st >= 2^32 - 1 is refused (-1, no launch). */
int evo_attn_decode_fp8(const void* q, const void* kv_data, const float* kv_scale, void* o,
                        int64_t B, int64_t H, int64_t Tk, int64_t q_sb, int64_t q_sh,
                        int64_t d_sb, int64_t d_st, int64_t d_sw, int64_t d_sh, int64_t s_sb, int64_t s_sw, int64_t s_sh,
                        const int64_t* dyn_pos, float* part_o, float* part_ml, int64_t n_splits,
                        float softmax_scale, void* stream);

/* ---- paged bf16 KV cache for decode (added under ABI 20, no signature changed; csrc/kv_paged.hip) ---------------------------------------
 * The two entries below stand where the reference calls flash_attn_with_kvcache  [REF evo/generation.py:138-155] on one contiguous
 * cache per sequence; the reference has no paged cache.  Opt-in (DecodePool(kv_paged=True)): the entries above are untouched.
 *   THE CACHE OPERAND of a layer (the same in both entries):
 *     pages [n_pages, page_tokens, 2, H, 128] bf16, 16-byte aligned, ELEMENT strides p_sp (page), p_st (token), p_sw (K | V), p_sh
 *           (head), each a multiple of 8 (p_st, p_sw, p_sh >= 128) -- inside a page the layout of evo_attn_decode_bf16's cache;
 *     table [B, table_width] int32, contiguous, 4-byte aligned: token t of row b lives in page table[b, t >> log2(page_tokens)], at
 *           row t & (page_tokens - 1) of it.  One table serves every layer of a model.
 *   page_tokens is a power of two >= 64 (a 64-key block of the streaming kernel then lies inside one page) with
 *   page_tokens * p_st * 2 < 2^32 - 1 (a lane's offset inside a page is 32-bit); n_pages >= 1, table_width >= 1.  A row holds at most
 *   table_width * page_tokens keys: there is no 4 GiB bound on a row or on the pool (the page base is 64-bit) and no second kernel form.
 *   Whatever the table holds, no access leaves the pool: the kernels clamp a table index to [0, table_width - 1] and a page id to
 *   [0, n_pages - 1].  By convention page 0 is a scrap page and every entry no live row owns is 0 (evo_amd/sh/cache.py PagedKV).
 *   Both return -1 without a launch on a null pointer, a misaligned pointer (16 bytes for data, 8 for pos, 4 for the table and f32
 *   vectors), a page_tokens, stride or count that breaks the rules above, or a size <= 0.
 *
 * evo_rope_append_decode_bf16 with the cache row found through the table: rotary on q and k of qkv [B, 3, H, 128] in place at pos[b]
 * -- the bits left in qkv are exactly that entry's, q_scale included -- then k (rotated) and v go to token pos[b] of row b's pages.
 * One launch, per-row device positions, capturable.  hd must be 128. */
int evo_rope_append_decode_paged_bf16(void* qkv, void* pages, const int32_t* table, const int64_t* pos, const float* inv_freq,
                                      float scaling, int64_t B, int64_t H, int64_t hd,
                                      int64_t page_tokens, int64_t n_pages, int64_t table_width,
                                      int64_t p_sp, int64_t p_st, int64_t p_sw, int64_t p_sh, float q_scale, void* stream);
/* evo_attn_decode_bf16's contract on paged keys: q [B, 1, H, 128] bf16 (q_sb, q_sh element strides), o [B, 1, H, 128] bf16 contiguous,
 * pos [B] device int64 (required): row b sees keys [0, pos[b]] and nothing behind them is read; the same part_o / part_ml workspace, the
 * same split partition (split s takes the 64-key blocks s, s + n_splits, ...; 1 <= n_splits <= 1024) and the same combine launch.
 * softmax_scale <= 0: pre-scaled queries.  The kernel (attn_decode_paged_kernel) is attn_decode_stream_kernel in everything that
 * produces a value, so for the same keys, positions and n_splits its output equals evo_attn_decode_bf16's bit for bit; a wave takes the
 * page ids of its next 64 blocks with one load per lane ahead of their use. */
int evo_attn_decode_paged_bf16(const void* q, const void* pages, const int32_t* table, void* o,
                               int64_t B, int64_t H, int64_t page_tokens, int64_t n_pages, int64_t table_width,
                               int64_t q_sb, int64_t q_sh, int64_t p_sp, int64_t p_st, int64_t p_sw, int64_t p_sh,
                               const int64_t* pos, float* part_o, float* part_ml, int64_t n_splits,
                               float softmax_scale, void* stream);

/* ---- FP8 (OCP e4m3fn) weights for the decode step at 1-8 rows (ABI 20; csrc/gemv_fp8.hip; no counterpart in the reference) -------------
 * Opt-in: the bf16 entries above are untouched and remain the default.  At 1-8 batch rows a decode step streams every dense weight
 * once and is bound by those bytes; these entries stream half of them.
 *
 * THE RULE (the KV cache's, ABI 19, with a weight row in place of a cache row; evo_amd/sh/cache.py fp8_row_rule states it in torch and
 * both sides agree bit for bit).  A row is the K values of one output feature n of a dense layer W [N, K].  With a = max_k |W[n, k]|, e is the
 * smallest integer with a 2^-e <= 448, clamped to [-126, 120]; a = 0 gives e = 0.  Stored: K bytes RNE_e4m3fn(W[n, k] 2^-e) and one
 * f32 scale 2^e.  Inputs are finite.  W 2^-e is exact in fp32 and at most 448 in magnitude, so the conversion rounds once and never
 * saturates; byte * scale is exact.  A dequantised row quantises to a record of the same VALUES (to the same bytes and scale unless its
 * scaled maximum rounded down to the byte 224: then to every byte doubled under half the scale).  The rule commutes with any permutation
 * of the rows: the grouped l1 | l2 order (evo_mlp_gate_mfma_bf16) needs no rule of its own.
 *
 * LAYOUT: w_data [N, K] uint8, row-major, 16-byte aligned; w_scale [N] f32.  K % 16 == 0: a lane's 16-byte load is 16 weights and
 * meets two of x's 16-byte vectors.
 *
 * ARITHMETIC: the bf16 kernels' on the bytes -- two bytes become a packed bf16 pair in registers (exactly: every e4m3fn value is a
 * bf16 value), v_dot2c_f32_bf16 accumulates in fp32 -- and the row's scale multiplies the REDUCED fp32 sum once per output element,
 * before bias, residual, gate or Hyena step.  With the rule's power-of-two scales that product is exact, so an entry returns what its
 * bf16 sibling's arithmetic returns on the dequantised weight, up to the order of the fp32 additions.  Scales that are no powers of
 * two are accepted and cost one more rounding per element.
 *
 * The compute entries take their bf16 siblings' arguments with (w_data, w_scale) in place of w, and return -1 without a launch on a
 * null or misaligned pointer (16 bytes; 4 for w_scale; bias / residual may be NULL where the sibling allows it), K % 16 != 0, M outside
 * 1-8, or a size <= 0.  Rows 9-64 (the MFMA forms) exist for bf16 weights only.
 *
 * evo_w_quant_fp8: w [N, K] bf16 -> w_data, w_scale by the rule; each row is read from memory once.  Nothing else is written. */
int evo_w_quant_fp8(const void* w, void* w_data, float* w_scale, int64_t N, int64_t K, void* stream);
/* evo_linear_small_m_bf16 at 1 <= M <= 8: y = x W^T (+ bias) (+ residual, which may alias y), one rounding.  ws / ws_bytes are the
 * sibling's workspace arguments and are not used (its 17-64-row forms have no FP8 counterpart). */
int evo_linear_small_m_w8(const void* x, const void* w_data, const float* w_scale, const void* bias, const void* residual, void* y,
                          int64_t M, int64_t N, int64_t K, void* ws, int64_t ws_bytes, void* stream);
/* evo_norm_linear_small_m_bf16: RMSNorm folded in front.  1 <= M <= 4 at any K, 5 <= M <= 8 at K = 4096 (the LDS-staged form), as the
 * sibling. */
int evo_norm_linear_small_m_w8(const void* x, const void* scale, const void* w_data, const float* w_scale, const void* bias, void* y,
                               int64_t M, int64_t N, int64_t K, float eps, void* stream);
/* evo_hyena_decode_fused_small_m: pre-norm + projection + FIR / modal step + gate, states updated in place.  Same rows as above, D = K. */
int evo_hyena_decode_fused_small_m_w8(const void* x, const void* norm_scale, const void* proj_data, const float* proj_scale,
                                      const void* proj_b, void* fir_state, float* iir_state, const void* fir_w, const void* fir_b,
                                      const float* poles, const float* residues, const void* dskip, void* y,
                                      int64_t M, int64_t D, int64_t n_heads, float eps, void* stream);
/* evo_mlp_gate_small_m_bf16's dot2 form: a = gelu(x W1^T) * (x W2^T), w12 = [W1; W2] plain or grouped (`grouped` != 0: I % 32 == 0).
 * 1 <= M <= 8 at any K (the sibling hands 5-8 rows to its MFMA form; here they stay on the dot2 stream). */
int evo_mlp_gate_small_m_w8(const void* x, const void* w12_data, const float* w12_scale, void* a, int64_t M, int64_t I, int64_t K,
                            int64_t grouped, void* stream);
/* evo_norm_mlp_gate_small_m_bf16: the same with RMSNorm folded in front; rows as evo_norm_linear_small_m_w8. */
int evo_norm_mlp_gate_small_m_w8(const void* x, const void* scale, const void* w12_data, const float* w12_scale, void* a,
                                 int64_t M, int64_t I, int64_t K, float eps, int64_t grouped, void* stream);

/* ---- FP8 weights at 5-64 rows: the MFMA weight-streaming forms (added under ABI 20, no signature changed; csrc/skinny_fp8.hip) ----------
 * The record, the rule and the layout are the ones above.  The kernels are the n-split forms of evo_linear_small_m_bf16 /
 * evo_mlp_gate_small_m_bf16 at 5-64 rows (csrc/skinny_nw.h) with one byte per weight to stream: the bytes of a chunk are requested as
 * contiguous row pieces, parked in LDS as bytes, converted to bf16 in registers (exactly) and multiplied against the bf16 x rows with
 * v_mfma_f32_16x16x32_bf16, fp32 accumulation.  The row's scale multiplies the reduced fp32 sum once per output element -- under a
 * split over K once per partial sum -- before bias, residual or gate; one rounding at the end.  With power-of-two scales an entry
 * returns what its sibling's arithmetic returns on the dequantised weight, up to the order of the fp32 additions.
 *
 * Both return -1 without a launch on a null or misaligned pointer (16 bytes; 4 for the scale; bias / residual / ws may be NULL),
 * M outside 5-64, K < 256 or K % 256 != 0, N < 1 (I < 32 or I % 32 != 0), or a size whose element counts leave 32-bit indices.
 *
 * evo_linear_skinny_w8: y [M, N] = x [M, K] W^T (+ bias [N]) (+ residual [M, N], which may alias y).  The dense layers of a decode
 * step [REF stripedhyena/model.py: projections, Wqkv, out_filter_dense, out_proj; layers.py ParallelGatedMLP.l3].  ws (16-byte
 * aligned, ws_bytes long, or NULL): with N < 8192, N % 64 == 0 and room for slices * M * N floats -- slices = min(8, K / 256,
 * ceil(256 / (N / 64))) >= 2 -- K is split across workgroups, the partial sums go through ws and a second launch adds them in slice
 * order; otherwise one launch, whole K per wave, any N.  Nothing but y and ws is written. */
int evo_linear_skinny_w8(const void* x, const void* w_data, const float* w_scale, const void* bias, const void* residual, void* y,
                         int64_t M, int64_t N, int64_t K, void* ws, int64_t ws_bytes, void* stream);
/* evo_mlp_gate_skinny_w8: a [M, I] = gelu(x W1^T) * (x W2^T) [REF stripedhyena/layers.py ParallelGatedMLP], w12 = [W1; W2] ([2 I, K])
 * plain, or (`grouped` != 0) in evo_mlp_gate_mfma_bf16's row order.  Both scaled sums are rounded to bf16, the gate is evaluated in
 * fp32 and rounded once: evo_mlp_gate_small_m_bf16's arithmetic at these rows.  Nothing but a is written. */
int evo_mlp_gate_skinny_w8(const void* x, const void* w12_data, const float* w12_scale, void* a, int64_t M, int64_t I, int64_t K,
                           int64_t grouped, void* stream);

/* decode behind SHARED prompts (ABI 15): row b attends to the keys [0, pre_len[pre_row[b]]) of row pre_row[b] of a prompt store and
 * then to its OWN keys [0, own_pos[b]] -- what evo_attn_decode_bf16 returns on the concatenation, without a copy of the prompt per
 * row (a decode pool that draws many samples from few prompts; no counterpart in the reference).
 *   q, k, v, o, B, H, Tk, strides: as above, k / v the rows' own caches (Tk their capacity); own_pos [B] device int64.
 *   k_pre / v_pre: views [R, P_cap, H, 128] of the store with element strides (row, token, head); pre_row [B] device int64: the store
 *   row a batch row continues, or -1 (none); pre_len [R] device int64: the keys each store row holds (>= 1 where referenced; values
 *   beyond P_cap are read as P_cap, rows >= R as -1).  Everything per row or per prompt is device memory: a captured step replays
 *   unchanged while slots are re-filled.
 *   part_o [B, H, n_pre_splits + n_splits, 128] f32, part_ml [.., 2] f32: splits [0, n_pre_splits) are the prefix -- split s takes the
 *   64-key blocks s, s + n_pre_splits, ... of the store row; a row without a prefix (or a split without a block) holds (m, l) =
 *   (-inf, 0) and zeros -- the remaining n_splits the own keys, partitioned as attn_decode_stream_kernel partitions them (it is that
 *   kernel, writing behind the prefix's splits).  One combine launch merges them all.
 *   Prefix kernel (attn_decode_group_kernel): a workgroup serves EVO_ATTN_GROUP_ROWS consecutive batch rows, a wave one split; for
 *   every DISTINCT store row among the tile's rows the wave streams that row's blocks once and updates the rows that name it.  Rows
 *   of one prompt placed next to each other read it once per tile; any other arrangement is as correct and reads more.
 *   Refused (-1, no launch): null pointers; R < 1; n_pre_splits < 1; n_splits < 1; n_pre_splits + n_splits > 1024; a stride that is
 *   not a multiple of 8; P_cap * kp_st * 2, P_cap * vp_st * 2, Tk * k_st * 2 or Tk * v_st * 2 at or above 2^32 - 1 (both kernels
 *   address keys with 32-bit offsets; this entry has no MFMA form to fall back on). */
#ifndef EVO_ATTN_GROUP_ROWS
#define EVO_ATTN_GROUP_ROWS 8
#endif
int evo_attn_decode_prefix_bf16(const void* q, const void* k, const void* v, void* o,
                                int64_t B, int64_t H, int64_t Tk,
                                int64_t q_sb, int64_t q_sh,
                                int64_t k_sb, int64_t k_st, int64_t k_sh,
                                int64_t v_sb, int64_t v_st, int64_t v_sh,
                                const int64_t* own_pos,
                                const void* k_pre, const void* v_pre, int64_t R, int64_t P_cap,
                                int64_t kp_sb, int64_t kp_st, int64_t kp_sh,
                                int64_t vp_sb, int64_t vp_st, int64_t vp_sh,
                                const int64_t* pre_row, const int64_t* pre_len,
                                float* part_o, float* part_ml, int64_t n_pre_splits, int64_t n_splits,
                                float softmax_scale, void* stream);

/* ---- skinny dense layer (decode) ----------------------------------------------------------------------
 * replaces cuBLAS GEMV-shaped nn.Linear calls of the single-token forward   [REF evo/generation.py:151-155]
 * y [M, N] = x [M, K] . w [N, K]^T (+ bias [N]) (+ residual [M, N]);  1 <= M <= 64 (ABI 10; 16 before), K % 8 == 0 (K % 32 == 0
 * for M > 8), all bf16, fp32 accumulate, one rounding.  Weight-streaming (HBM-bound) forms: dot2 on the VALU up to
 * M = 4, v_mfma_f32_16x16x32_bf16 with the batch rows on the MFMA's N side from M = 5 -- one to four tiles of 16 rows per weight pass
 * (17-64 rows: the pooled decode step of 17-64 live streams); `residual` may alias `y`.  From 5 rows on layers with N >= 8192 and K % 256 == 0 the
 * weight is requested in whole 512-byte row pieces and the x rows of a 256-k chunk are shared by the workgroup's waves through LDS (csrc/gemv.hip
 * skinny_nw_kernel).  `ws` (ABI 10; may be NULL): a 16-byte aligned fp32 workspace of `ws_bytes` >= 8 M N 4 bytes lets the narrow layers (N < 8192) at
 * 17-64 rows split K over workgroups -- partial sums through ws, added in a fixed order by a second small launch; without it they run the k-split form. */
int evo_linear_small_m_bf16(const void* x, const void* w, const void* bias, const void* residual, void* y,
                            int64_t M, int64_t N, int64_t K, void* ws, int64_t ws_bytes, void* stream);

/* ---- dense layer on the MFMA pipe (prefill) --------------------------------------------------------------
 * replaces the cuBLAS nn.Linear GEMMs of the attention block: Wqkv (with bias) and out_proj (+ residual)
 *                                                     [REF stripedhyena/model.py:52-59 (MHA projections), :84-92]
 * y [M, N] = x [M, K] . w [N, K]^T (+ bias [N]) (+ residual [M, N]); all bf16, fp32 accumulate on
 * v_mfma_f32_32x32x16_bf16, one rounding.  N % 256 == 0, K % 64 == 0, any M >= 1 (ragged last row tile);
 * `residual` may alias `y`; `x` must not alias `y`.  Returns -1 for an unsupported shape. */
int evo_linear_mfma_bf16(const void* x, const void* w, const void* bias, const void* residual, void* y,
                         int64_t M, int64_t N, int64_t K, void* stream);

/* ---- gated MLP, first half, on the MFMA pipe (prefill) ----------------------------------------------------------
 * replaces l1 / l2 (two nn.Linear GEMMs) + F.gelu + the elementwise product of ParallelGatedMLP.forward
 *                                                     [REF stripedhyena/layers.py ParallelGatedMLP: l3(gelu(l1 x) * l2 x)]
 * a [M, I] = gelu(x [M, K] . W1^T) * (x . W2^T), all bf16; z1 = x W1^T and z2 = x W2^T are rounded to bf16 (the dense layers'
 * outputs in the reference), the exact-erf gate is evaluated in fp32 and rounded once -- the arithmetic of evo_gelu_gate_bf16
 * behind evo_linear_mfma_bf16, bit for bit, without the [M, 2 I] intermediate.  `w12g` = the 2 I rows of [W1; W2] regrouped in
 * blocks of 64: rows 32 q .. 32 q + 31 of W1 followed by the same rows of W2 (q = 0 .. I / 32 - 1).
 * (2 I) % 256 == 0, K % 64 == 0, K >= 128, any M >= 1.  Returns -1 for an unsupported shape. */
int evo_mlp_gate_mfma_bf16(const void* x, const void* w12g, void* a, int64_t M, int64_t I, int64_t K, void* stream);

/* ---- RMSNorm folded into the dense layers around it (prefill-sized batches) ---------------------------------------------
 * replaces the RMSNorm pass between two dense layers          [REF stripedhyena/model.py: pre_norm / post_norm of every block;
 *                                                              stripedhyena/layers.py RMSNorm.forward]
 * The reference writes n = bf16(g * x / (rms(x) + eps)) and multiplies it by the next layer's weight W.  Here the dense layer that
 * WRITES the residual stream x also emits each row's sum of squares, and the layer that consumes the norm reads x itself:
 *     W n  =  r_m * ((W diag(g)) x_m),   r_m = 1 / (rms(x_m) + eps)
 * with W diag(g) a bf16 copy of the weight the caller folds once (one rounding of the weight where the reference rounds the
 * activation) and r_m applied to the fp32 accumulators before bias / gate / the one output rounding.
 *   sumsq  [N / 128][ss_ld] fp32 out: per 128-column strip of the stored rows, the sum of squares of the ROUNDED values of row m
 *          (ss_ld >= M rounded up to 256; rows beyond M are scratch).  Needs `residual` (the launches that write the stream).
 *   row_scale [M rounded up to 256] fp32 in: r_m.  Launches without a residual.
 *   evo_rms_finalize_f32: rstd[m] = 1 / (sqrt(sum over strips) / sqrt(D) + eps) for m < M_main (strip order: bit-reproducible), and
 *          computed from the rows of x [M, D] bf16 themselves for M_main <= m < M (the rows a weight-streaming launch wrote).
 *   evo_linear_t_mfma_nf_bf16: additionally reads its token rows from the stream in (batch row, token) order: position p = b Tm + t
 *          of z^T (Mp = B Tm, Tm % 256 == 0) is row p + b row_skip of x [x_rows, K] -- the tail form of z^T; row_scale has x_rows
 *          entries.  row_scale == NULL: the plain launch (x_rows = Tm = Mp, row_skip = 0).
 * Shape contracts as the plain entries'; K >= 128 and operands below 4 GiB (the persistent kernel). */
int evo_linear_mfma_nf_bf16(const void* x, const void* w, const void* bias, const void* residual, void* y,
                            const float* row_scale, float* sumsq, int64_t ss_ld, int64_t M, int64_t N, int64_t K, void* stream);
int evo_linear_xblk_mfma_nf_bf16(const void* x_blk, const void* w, const void* bias, const void* residual, void* y,
                                 float* sumsq, int64_t ss_ld, int64_t M, int64_t N, int64_t K, void* stream);
int evo_mlp_gate_mfma_nf_bf16(const void* x, const float* row_scale, const void* w12g, void* a, int64_t M, int64_t I, int64_t K, void* stream);
int evo_linear_t_mfma_nf_bf16(const void* x, const float* row_scale, const void* w, const void* bias, void* zt, int64_t Mp, int64_t N,
                              int64_t K, int64_t x_rows, int64_t Tm, int64_t row_skip, void* stream);
int evo_rms_finalize_f32(const float* sumsq, int64_t n_strips, int64_t ss_ld, const void* x, int64_t M_main, int64_t M, int64_t D,
                         float eps, float* rstd, void* stream);

/* ---- Hyena mixer input of one decode step, fused ---------------------------------------------------------------
 * replaces pre-norm + projections GEMV + step_fir + step_iir of the single-token forward   [REF evo/generation.py:111-114,138-155]
 * x [M, D] bf16 residual rows (M = batch, 1 <= M <= 4; up to 8 at D = 4096), norm_scale [D], proj_w [3D, D], proj_b [3D] -> y [M, D] bf16;
 * fir_state [M, 3D, 2] bf16 and iir_state [M, D, 8] complex64 are updated in place.  Bit-identical to
 * evo_norm_linear_small_m_bf16 followed by evo_hyena_step. */
int evo_hyena_decode_fused_small_m(const void* x, const void* norm_scale, const void* proj_w, const void* proj_b,
                                   void* fir_state, float* iir_state, const void* fir_w, const void* fir_b,
                                   const float* poles, const float* residues, const void* dskip, void* y,
                                   int64_t M, int64_t D, int64_t n_heads, float eps, void* stream);

/* ---- RMSNorm + dense layer, decode form ----------------------------------------------------------------------
 * replaces the pre-mixer RMSNorm and the projection GEMV of the single-token forward     [REF evo/generation.py:151-155;
 *                                                                                   evo/configs/evo-1-8k-base_inference.yml:13]
 * y [M, N] = bf16(scale * x / (rms(x) + eps)) . w [N, K]^T (+ bias [N]);  1 <= M <= 4 (up to 8 at K = 4096), K % 8 == 0,
 * all bf16.  The
 * normalised row is bit-identical to what evo_rmsnorm_bf16 stores (same reduction order). */
int evo_norm_linear_small_m_bf16(const void* x, const void* scale, const void* w, const void* bias, void* y,
                                 int64_t M, int64_t N, int64_t K, float eps, void* stream);

/* ---- gated MLP input, decode form ---------------------------------------------------------------------------
 * replaces the l1 / l2 GEMV pair + gelu * mul of the single-token forward   [REF evo/configs/evo-1-8k-base_inference.yml:38;
 *                                                                          evo/generation.py:151-155]
 * a [M, I] bf16 = gelu_erf(x . W1^T) * (x . W2^T) with w12 [2I, K] = [W1; W2] bf16, x [M, K] bf16; 1 <= M <= 4,
 * I % 2 == 0, K % 8 == 0.  Both products are rounded to bf16 before the gate, as the unfused layers store them.
 * `grouped` != 0 (ABI 10): w12 is given in the row order of evo_mlp_gate_mfma_bf16's w12g -- blocks of 64 rows = 32 rows of W1 followed
 * by the same 32 rows of W2 (I % 32 == 0) -- so that ONE copy of l1 | l2 serves the prefill launch and the decode launches.
 * 5 <= M <= 64 (ABI 10; I % 32 == 0, K % 256 == 0, either layout): the MFMA weight-streaming form with the gate in its epilogue (csrc/gemv.hip
 * skinny_nw_kernel GATE) -- the pooled decode step of 5-64 live streams and the BOS sliver rows of a scoring batch; bit for bit
 * evo_linear_small_m_bf16 on w12 followed by evo_gelu_gate_bf16. */
int evo_mlp_gate_small_m_bf16(const void* x, const void* w12, void* a, int64_t M, int64_t I, int64_t K, int64_t grouped, void* stream);
/* same with the post-mixer RMSNorm folded in: x is the residual row, `scale` [K] the norm weight (bit-identical to
 * evo_rmsnorm_bf16 followed by evo_mlp_gate_small_m_bf16); this form also takes 5 <= M <= 8 at K = 4096. */
int evo_norm_mlp_gate_small_m_bf16(const void* x, const void* scale, const void* w12, void* a, int64_t M, int64_t I,
                                   int64_t K, float eps, int64_t grouped, void* stream);

/* ---- gated MLP activation ---------------------------------------------------------------------------
 * replaces ATen gelu + mul                                  [REF evo/configs/evo-1-8k-base_inference.yml:38]
 * g [M, 2*I] bf16 = [l1 x | l2 x]  ->  a [M, I] bf16 = gelu_erf(g[:, :I]) * g[:, I:]. */
int evo_gelu_gate_bf16(const void* g, void* a, int64_t M, int64_t I, void* stream);

/* ---- scoring tail ---------------------------------------------------------------------------------------
 * replaces torch.log_softmax + gather (+ entropy)            [REF evo/scoring.py:47-57,119-121]
 * logits [M, V] bf16 (logits_f32 = 0) or f32 (logits_f32 = 1; evo.generation keeps its score buffer in
 * f32 [REF evo/generation.py:97-103,287]), target [M] int64 (0 is written where target < 0 or >= V)
 * -> logprob [M] f32 (may be NULL), entropy [M] f32 (may be NULL).  fp32 log-softmax. */
int evo_logprob_entropy(const void* logits, int64_t logits_f32, const int64_t* target, float* logprob,
                        float* entropy, int64_t M, int64_t V, void* stream);

/* ---- fused scoring tail: unembed + log_softmax + gather (+ entropy) ---------------------------------
 * replaces  logits = x @ E^T ; log_softmax(logits) ; gather(next token) ; -sum p log p
 *                                                         [REF evo/scoring.py:47-57,81-84,119-121]
 * hidden [M, K] bf16 (final-norm output), emb [V = 512, K] bf16 (tied embedding), target [M] int64 or
 * NULL (negative = masked -> log-prob 0), logprob / entropy [M] f32 or NULL.  The [M, V] logits are
 * never written to HBM; every logit is rounded to bf16 once (the reference's logits tensor is bf16)
 * and the softmax statistics are taken in fp32 on the rounded values.  V must be 512, K % 32 == 0. */
int evo_unembed_logprob_bf16(const void* hidden, const void* emb, const int64_t* target,
                             float* logprob, float* entropy, int64_t M, int64_t V, int64_t K, void* stream);

/* ---- fused scoring tail with a per-row profile: the log-probs of chosen vocabulary ids --------------------------
 * replaces  log_softmax(x @ E^T)[:, sel]  next to the gather and the entropy above -- what a user asks of a DNA model at every
 * position: the log-probability of A, C, G and T (substitution scores, the predicted base)   [REF evo/scoring.py:47-57,119-121]
 * The same kernel body as evo_unembed_logprob_bf16 (k-loop, one bf16 rounding of every logit, fp32 max / sum-exp) with a second
 * epilogue; hidden, emb, target, logprob, entropy, M, V, K exactly as there (target may be NULL; a target outside [0, 512) gives
 * log-prob 0; logprob / entropy may be NULL), bit for bit the values that entry writes.
 *   sel          n_sel int32 ids in HOST memory, read at launch: they travel in the kernel arguments, so there is no device buffer,
 *                no device read and no alignment contract.  1 <= n_sel <= 8, every id in [0, 512), no id twice
 *   sel_logprob  [M, n_sel] f32 row-major (16-byte aligned base; rows of n_sel * 4 bytes):
 *                sel_logprob[m][j] = logit[m][sel[j]] - max_m - log sum_v exp(logit[m][v] - max_m), written for EVERY row, masked or not
 * The [M, V] logits are never written to HBM.  Returns -1 before any launch for V != 512, K % 32 != 0, n_sel outside 1 .. 8, a NULL
 * sel or sel_logprob, an id outside [0, 512) or a repeated id. */
int evo_unembed_profile_bf16(const void* hidden, const void* emb, const int64_t* target, const int32_t* sel, int64_t n_sel,
                             float* sel_logprob, float* logprob, float* entropy, int64_t M, int64_t V, int64_t K, void* stream);

/* ---- sequence embeddings: masked row pooling (+ fused RMSNorm) --------------------------------------------
 * replaces the torch mean over positions of the hidden states that evo users take as embeddings (no reference kernel: upstream
 * users swap in an identity unembedding and reduce [B, T, D] in eager torch)
 *   x      [M, D] bf16 rows with a pitch of `ld` elements (ld >= D, ld % 8 == 0, x 16-byte aligned): the residual stream
 *   ranges [B, 2] device int64: sequence b pools rows first_b .. first_b + n_b - 1 of x (a range with first_b < 0, n_b < 1 or
 *          first_b + n_b > M pools nothing and gets a NaN row; the test is n_b <= M - first_b, so no int64 pair can wrap past it)
 *   scale  [D] bf16 or NULL: with it f(x) = scale * x / (||x||_2 D^-1/2 + eps) (the engine's RMSNorm, eps outside the root) taken
 *          in fp32 from the bf16 rows, no rounding in between; NULL: f(x) = x.  The scale is applied once, after the sum.
 *   mode   0 = mean:  out[b] = (1 / n_b) * sum_t f(x_t);  1 = last:  out[b] = f(x_{first_b + n_b - 1})
 *   ws     fp32 workspace of B * n_strips * D floats (B * n_strips * D * 4 bytes): one partial slab per (sequence, strip); a
 *          sequence's rows are split into n_strips nearly equal strips, one workgroup each (1 <= n_strips <= 65535)
 *   out    [B, D] fp32
 * Two launches (strip partials, then a fixed-order sum of each sequence's slabs), no float atomics: bit-identical from run to run.
 * D <= 4096 (the register plan: D / 64 fp32 column sums per lane), D % 8 == 0, 1 <= B <= 65535.  Returns -1 for a null pointer
 * (x, ranges, ws, out), a bad D / ld / M, B < 1, n_strips out of range or an unknown mode. */
int evo_pool_rows_bf16(const void* x, int64_t M, int64_t D, int64_t ld, const int64_t* ranges, int64_t B,
                       const void* scale, float eps, int64_t mode, int64_t n_strips, float* ws, float* out, void* stream);

/* ---- seeded sampling: one token per row of [S, 512] logits, on the device -------------------------------------
 * replaces stripedhyena.sample (topk / sort / softmax / cumsum / scatter / masked_fill_ / multinomial in eager torch, the logits
 * and the sampled ids read back by the host every step)     [REF evo/generation.py:7,162-167; semantic_design/semantic_design.py:121-179]
 * One launch, no host reads, no allocation: capturable in a hipGraph.  Written specification: evo_amd/sh/sample.py sample_seeded.
 *   logits      [S, V = 512] bf16 (logits_f32 = 0) or f32 (logits_f32 = 1), row pitch `ld` elements (ld >= 512, ld % 8 == 0, 16-byte aligned)
 *   top_k       [S] device int32: 1 = arg-max (lowest id on ties); > 1: keep logits >= the k-th largest (ties kept); <= 0: keep all
 *   top_p       [S] device f32: with 0 < top_p < 1 drop, in ascending order, while the cumulative softmax is <= 1 - top_p
 *   temperature [S] device f32: the kept logits are divided by it unless it is 1 or <= 0
 *   allow       64 device bytes or NULL: bit j of byte b set = token 8 b + j may be drawn (others count as -inf); NULL = all
 *   seed, stream_id [S] int64 (NULL: the row index), count [S] int64 (NULL: 0): the row's random number is word 0 of Philox4x32-10 with
 *               key (seed low, seed high) and counter (stream low, stream high, count low, count high), u = ((x0 >> 8) + 0.5) 2^-24;
 *               the token is the first one, by descending logit and ascending id, whose inclusive CDF over the kept set exceeds u
 *   active      [S] device bytes or NULL: a row whose byte is 0 writes nothing and does not advance
 *   ids_out     [S] int64;  logprob_out [S] f32: log-probability of the token under the fp32 log-softmax of the UNFILTERED row
 *   hist_ids    [S, hist_len] int64 or NULL, hist_logits [S, hist_len, 512] f32 or NULL (16-byte aligned): with 0 <= count[s] < hist_len,
 *               hist_ids[s, count[s]] = token and hist_logits[s, count[s], :] = the row in f32 (outside that range nothing is recorded)
 *   then count[s] += 1 (when count is given).
 *   Alignment: logits and hist_logits 16 bytes (above); the per-row vectors (top_k, top_p, temperature, stream_id, count, active,
 *   ids_out, logprob_out, hist_ids) are read and written one element per row and need only that element's own alignment -- the
 *   decode pool samples ONE slot by passing one-element slices of its per-slot vectors.
 * fp32 sums in a fixed order, no float atomics: bit-identical from run to run.  Returns -1 for a null logits / top_k / top_p /
 * temperature / ids_out / logprob_out, S < 1, V != 512, a bad ld or alignment, or history without count or with hist_len < 1. */
int evo_sample_rows_f32(const void* logits, int64_t logits_f32, int64_t ld, const int32_t* top_k, const float* top_p,
                        const float* temperature, const void* allow, uint64_t seed, const int64_t* stream_id, int64_t* count,
                        const uint8_t* active, int64_t* ids_out, float* logprob_out, int64_t* hist_ids, float* hist_logits,
                        int64_t hist_len, int64_t S, int64_t V, void* stream);

/* ---- seeded sampling with job control: the row itself decides that its job is over ---------------------------------
 * no reference counterpart in the pooled form; the single-stream rule it generalises is the reference's stop at EOS
 *                                                            [REF evo/generation.py:136-139; semantic_design/semantic_design.py:121-179]
 * Call site: DecodePool's job-control path (evo_amd/pool.py: _sample_rows_ctl, the last node of the captured pooled step and the
 * one-row launch that draws a job's first token from its prefill's logits).  Written specification: evo_amd/sh/sample.py
 * finish_reason / sample_ctl.  One launch, no host reads, no allocation, plain vector stores, no float atomics: capturable.
 * The draw is evo_sample_rows_f32's own device code: on the same inputs token, logprob_out, hist_ids and hist_logits are bit-identical.
 * Everything evo_sample_rows_f32 takes means what it means there, except:
 *   count, active   required.  active [S] device bytes is now in/out: the kernel clears a row's byte when its job ends
 *   hist_ids [S, hist_len] int64, hist_logits [S, hist_len, 512] f32 (16-byte aligned), hist_logprob [S, hist_len] f32: each one
 *               optional on its own; what is given is recorded at [s, count[s]] (hist_logprob: the value of logprob_out)
 *   limit       [S] device int64: the job's length limit
 *   stop_mask   64 device bytes in allow's layout or NULL: the stop tokens
 *   stop_seq    HOST int32 [n_seq, 8], stop_seq_len HOST int32 [n_seq], 0 <= n_seq <= 8, every length in 1 ... 8: the stop patterns.
 *               They are read before the launch and travel in its arguments (a captured graph keeps the patterns it was captured with)
 *   stop_frame  >= 1
 *   length      [S] device int64, finish [S] device bytes: written only when a job ends
 * Per active row, with cnt = count[s]:
 *   cnt < 0, cnt >= limit[s], or (with any history) cnt >= hist_len: active[s] = 0, length[s] = cnt, finish[s] = 3; nothing is drawn,
 *   neither the logits nor the history are read, count stays.
 *   Otherwise the token is drawn and recorded, n = count[s] = cnt + 1, and the FIRST reason that holds ends the job:
 *     1  the token's bit is set in stop_mask
 *     2  n % stop_frame == 0 and for some pattern p of length l <= n the last l recorded tokens (the new one included) equal p.  Lane 0
 *        compares the new token and then hist_ids[s, cnt - 1 ... cnt - l + 1] (>= 0: a pattern longer than n reads nothing), which earlier
 *        launches on the same stream wrote
 *     3  n >= limit[s]
 *   and then active[s] = 0, length[s] = n, finish[s] = the reason.  The token that ends a job is part of it.
 * Inactive rows write nothing.  Returns -1 for everything evo_sample_rows_f32 refuses, a null count / active / limit / length / finish,
 * n_seq outside 0 ... 8, n_seq > 0 with a null stop_seq / stop_seq_len / hist_ids, a pattern length outside 1 ... 8, stop_frame < 1, or
 * a history with hist_len < 1. */
#define EVO_SAMPLE_MAX_STOP_SEQ 8
#define EVO_SAMPLE_MAX_STOP_LEN 8
int evo_sample_rows_ctl_f32(const void* logits, int64_t logits_f32, int64_t ld, const int32_t* top_k, const float* top_p,
                            const float* temperature, const void* allow, uint64_t seed, const int64_t* stream_id, int64_t* count,
                            uint8_t* active, int64_t* ids_out, float* logprob_out, int64_t* hist_ids, float* hist_logits,
                            float* hist_logprob, int64_t hist_len, const int64_t* limit, const void* stop_mask,
                            const int32_t* stop_seq, const int32_t* stop_seq_len, int64_t n_seq, int64_t stop_frame,
                            int64_t* length, uint8_t* finish, int64_t S, int64_t V, void* stream);

/* ---- seeded sampling with job control under a per-row token automaton: constrained generation --------------------------
 * no reference counterpart (the reference samples freely; a template, a fixed protein or an open reading frame is enforced there by
 * sampling and discarding)                                  [REF evo/generation.py:162-167; semantic_design/semantic_design.py:121-179]
 * Call site: DecodePool's job-control path when `constraints` is given (evo_amd/pool.py: _sample_rows_ctl, the last node of the captured
 * pooled step and the one-row launch that draws a job's first token).  Written specification: evo_amd/sh/sample.py dfa_allowed /
 * sample_dfa.  One launch, no host reads, no allocation, no LDS beyond the draw's, plain vector stores, no atomics: capturable.
 * Every argument of evo_sample_rows_ctl_f32 up to `finish` means what it means there.  In addition:
 *   dfa_alphabet HOST int32 [n_sym], 1 <= n_sym <= 8 distinct token ids in [0, 512): the symbols.  Read before the launch, they travel
 *               in its arguments (a captured graph keeps the alphabet it was captured with)
 *   dfa_next    device int32 [n_states, 8], 16-byte aligned, row pitch 8 always: row q, column a is what drawing dfa_alphabet[a] in
 *               state q does: >= 0 the next state (relative to the row's base), EVO_DFA_ACCEPT (-2) the constraint is complete, -1 (or
 *               any other negative value) forbidden.  Columns >= n_sym are ignored.  1 <= n_states <= 2^27
 *   dfa_base    device int64 [S]: the table row of the row's state 0; < 0 = the row is unconstrained
 *   dfa_state   device int32 [S], in/out: the row's state, relative to its base
 * Per active row, after evo_sample_rows_ctl_f32's own "nothing left to draw" check (unchanged: finish 3, no draw):
 *   dfa_base[s] < 0: exactly evo_sample_rows_ctl_f32; dfa_state[s] is neither read nor written.
 *   Otherwise r = dfa_base[s] + dfa_state[s].  With dfa_state[s] < 0, r outside [0, n_states), or no token both permitted by row r
 *   and by `allow`, the row is at a DEAD END: active[s] = 0, length[s] = cnt, finish[s] = 5; nothing is drawn, nothing else is read or
 *   written, count and dfa_state stay.
 *   Otherwise the token is drawn from {dfa_alphabet[a] : next[r][a] >= 0 or == EVO_DFA_ACCEPT} intersected with `allow`, by
 *   evo_sample_rows_ctl_f32's own device code: on the same logits and counters token, logprob_out (under the UNFILTERED row) and the
 *   histories are bit-identical to that entry called with this set packed as its 64 allow bytes.  Then lane 0, with a the symbol drawn
 *   and nxt = next[r][a]: nxt == EVO_DFA_ACCEPT leaves dfa_state[s] and makes reason 4 a candidate; otherwise dfa_state[s] = nxt.
 *   The FIRST reason that holds ends the job: 1 stop token, 2 in-frame stop pattern, 4 constraint accepted, 3 n >= limit[s]; then
 *   active[s] = 0, length[s] = n, finish[s] = the reason.  The token that ends a job is part of it.
 * Inactive rows write nothing.  dfa_base and dfa_state need only their element's alignment (one-element slices, as the other per-row
 * vectors).  Returns -1 for everything evo_sample_rows_ctl_f32 refuses, a null dfa_alphabet / dfa_next / dfa_base / dfa_state, n_sym
 * outside 1 ... 8, an alphabet id outside [0, 512) or given twice, n_states < 1 or > 2^27, or dfa_next not 16-byte aligned. */
#define EVO_DFA_MAX_SYMBOLS 8
#define EVO_DFA_MAX_STATES (1 << 27)
#define EVO_DFA_ACCEPT (-2)
int evo_sample_rows_dfa_f32(const void* logits, int64_t logits_f32, int64_t ld, const int32_t* top_k, const float* top_p,
                            const float* temperature, const void* allow, uint64_t seed, const int64_t* stream_id, int64_t* count,
                            uint8_t* active, int64_t* ids_out, float* logprob_out, int64_t* hist_ids, float* hist_logits,
                            float* hist_logprob, int64_t hist_len, const int64_t* limit, const void* stop_mask,
                            const int32_t* stop_seq, const int32_t* stop_seq_len, int64_t n_seq, int64_t stop_frame,
                            int64_t* length, uint8_t* finish, const int32_t* dfa_alphabet, int64_t n_sym,
                            const int32_t* dfa_next, int64_t n_states, const int64_t* dfa_base, int32_t* dfa_state,
                            int64_t S, int64_t V, void* stream);

/* ---- k-mer repeat control in front of the sampler launch (added under ABI 20, no signature changed; csrc/repeat.hip) ----
 * no device counterpart in the reference: its design pipeline generates, then discards sequences whose most frequent k-mer covers too much
 * of them, and its generation script hands a token-level repetition_penalty to the sampler
 *                                                           [REF semantic_design/semantic_design.py:565-590,613; scripts/generation_to_folding.py:43,94]
 * Call site: DecodePool's job-control path when `repeat` is given (evo_amd/pool.py: _repeat_rows, the node in front of the sampler launch of
 * the captured pooled step, and the one-row launch in front of the one that draws a job's first token).  Written specification:
 * evo_amd/sh/sample.py repeat_fold / repeat_ended / repeat_penalise / repeat_row.  One launch, one 64-lane wave per row, no host reads, no
 * allocation, no LDS, plain vector stores, no atomics: capturable.
 *   logits      [S, 512] bf16, or f32 with logits_f32 != 0; row pitch ld (>= 512, a multiple of 8); 16-byte aligned.  Read only
 *   out         f32 [S, 512], 16-byte aligned, row pitch 512: the row the sampler launch that follows draws from
 *   fed_ids     device int64 [S] or NULL: the token this step is fed (the one the previous step drew).  NULL: nothing is folded (a job's
 *               first row, computed from the prefill's last logits)
 *   active      device bytes [S]: rows with 0 read and write nothing
 *   counts      device int32 [S, M], in/out: how often each k-mer has been seen (saturating at 2^31 - 1)
 *   ctx         device int32 [S, 2], in/out: (code, len), the last len <= k - 1 alphabet symbols in base n_sym, newest in the lowest digit.
 *               A window outside its invariants (len outside [0, k - 1], code outside [0, M / n_sym)) reads as the empty one (0, 0): no index
 *               ever leaves the row's M cells
 *   stat        device int64 [S, 2], in/out: (n_gen, rep), the generated tokens folded in and how many of them completed a k-mer seen before
 *   levels      device f32 [S, 8]: what is subtracted at a count of 0 ... 7 (or more); the caller keeps levels[s][0] == 0
 *   end_num     device int32 [S] or NULL: the early end is armed for rows with end_num[s] > 0 (a fraction end_num / 1024); NULL: for none
 *   end_min_tokens  >= 1 when end_num is given
 *   count       device int64 [S], read only: the tokens the row's job has recorded (the sampler's counter); length / finish as the sampler's
 *   alphabet    HOST int32 [n_sym], 1 <= n_sym <= 8 distinct token ids in [0, 512).  Read before the launch, it travels in its arguments (a
 *               captured graph keeps the alphabet it was captured with), exactly as dfa_alphabet
 *   k >= 1, M == n_sym ** k <= 2^20
 * Per ACTIVE row, in this order (a = the symbol index of the token, if it is one):
 *   1. with fed_ids: no symbol: ctx = (0, 0).  A symbol at len == k - 1: idx = code * n_sym + a, old = counts[idx], counts[idx] =
 *      min(old + 1, 2^31 - 1), rep += 1 if old >= 1, code = idx % (M / n_sym).  A symbol at len < k - 1: code = code * n_sym + a, len += 1.
 *      n_gen += 1 in every case.  (k == 1: len == 0 == k - 1 always and idx = a: a per-token count.)
 *   2. with end_num: if end_num[s] > 0 and n_gen >= end_min_tokens and rep * 1024 > end_num[s] * n_gen (int64): active[s] = 0, length[s] =
 *      count[s], finish[s] = EVO_FINISH_REPEAT; out[s] is NOT written (the sampler launch skips the row).
 *   3. otherwise out[s] = the row widened to f32 (exact) and, if len == k - 1, for every symbol a: c = counts[code * n_sym + a] and
 *      out[s][alphabet[a]] -= levels[s][min(max(c, 0), 7)] -- ONE f32 subtraction, no multiply.  Every other id, and the whole row when
 *      len < k - 1, is the widened value bit for bit.
 * The per-row vectors need only their element's alignment (one-row slices).  Returns -1 before any launch, without dereferencing a device
 * pointer, for: a null logits / out / active / counts / ctx / stat / levels / alphabet; logits or out not 16-byte aligned, another operand
 * not aligned to its element; n_sym outside 1 ... 8; an alphabet id outside [0, 512) or given twice; k < 1; M != n_sym ** k or M > 2^20;
 * V != 512; ld < V or ld % 8 != 0; S < 1; end_num given with a null count / length / finish or end_min_tokens < 1. */
#define EVO_REPEAT_V 512
#define EVO_REPEAT_MAX_SYMBOLS 8
#define EVO_REPEAT_MAX_TABLE (1 << 20)
#define EVO_REPEAT_LEVELS 8
#define EVO_FINISH_REPEAT 6
int evo_repeat_rows_f32(const void* logits, int64_t logits_f32, int64_t ld, float* out, const int64_t* fed_ids, uint8_t* active,
                        int32_t* counts, int32_t* ctx, int64_t* stat, const float* levels, const int32_t* end_num, int64_t end_min_tokens,
                        const int64_t* count, int64_t* length, uint8_t* finish, const int32_t* alphabet, int64_t n_sym, int64_t k,
                        int64_t M, int64_t S, int64_t V, void* stream);

/* ---- beam search on the device (csrc/beam.hip; specification: evo_amd/sh/sample.py beam_select) ----------------
 * evo_beam_select_f32: one step of beam search over logits [S, 512] (bf16, or f32 with logits_f32 != 0; row stride ld), one launch,
 *   nothing read back: capturable.  A prompt owns a GROUP of W consecutive slots g W ... g W + W - 1, 1 <= W <= EVO_BEAM_MAX_WIDTH;
 *   G = S / W groups.  Slots >= G W and the slots of a group with group_active[g] == 0 (group_active NULL: every group is active) get
 *   parent[s] = s and nothing else is written for them.  Per-slot state, in / out: cum [S] f32 (sum of log-probabilities; -inf: the beam
 *   is EMPTY), ended [S] bytes, length [S] int64, ids [S] int64 (the token the next step feeds).  Per active group:
 *     a live beam b (cum > -inf, not ended) offers (b, v) for every token v of `allow` (64 bytes, bit j of byte i: token 8 i + j; NULL:
 *     all) with score cum[b] + (x[b][v] - lse[b]) in f32 in exactly that association, lse[b] the log-sum-exp of the UNFILTERED row by
 *     the sampler entries' own device code; an ended beam offers itself (score, ids, length unchanged; it stays ended); an empty beam
 *     offers nothing; a score that is NaN or -inf is no candidate.  Candidates rank by score descending (-0 = +0), then parent
 *     ascending, then token ascending.  Slot g W + j receives the j-th: parent (a slot index), ids = token, cum = score, length =
 *     length[parent] + (0 if the parent had ended, else 1), ended = parent ended or token in `stop_mask` (64 bytes as `allow`, or NULL).
 *     With fewer than W candidates the remaining slots become empty: parent = s, cum = -inf, ended = 0, ids and length unchanged.
 *   All of a group's state is read before any of it is written (one barrier; only the group's first wave writes).
 *   History: the step's column is step[g] when `step` (device int64 [G]) is given -- the launch then also writes step[g] + 1 back -- and
 *   the scalar t otherwise; with a column in [0, hist_len) the launch records hist_parent[s][col] (int32), hist_ids[s][col] (int64) and,
 *   when hist_cum is given, hist_cum[s][col] (f32) for the W slots of every active group ([S, hist_len] each).  t < 0 without `step`:
 *   nothing is recorded and the history operands are ignored.
 *   Returns -1 before any launch for: a null logits / cum / ended / length / ids / parent; logits not 16-byte aligned or another operand
 *   not aligned to its element; W outside 1 ... 8; S < W or S > 2^31 - 1; V != 512; ld < V or ld % 8 != 0; a step to record (t >= 0, or
 *   `step` given) with a null hist_parent or hist_ids or hist_len < 1.
 * evo_gather_rows: the reparenting copy.  For every slot s with p = clamp(parent[s], 0, S - 1) != s, row p of every tensor of `table`
 *   goes to row s -- OUT to the slot's scratch row (back == 0) and BACK from it (back == 1): the caller launches both, in that order, so
 *   that no row is read after it may have been written.  `table`: device int64 [n_entries][EVO_GATHER_FIELDS] = (base address, row
 *   stride in bytes, bytes of a row, bytes per token, offset in a scratch row, 0).  Bytes per token 0: the whole row moves; > 0: only
 *   the first own_pos[p] + 1 tokens (clamped to the row; own_pos: device int64 [S]).  Every address, stride, size and offset is a
 *   multiple of 16 (16-byte vector loads and stores); bytes beyond what moves, and slots with parent[s] == s, are untouched.  A copy
 *   never leaves the slot's scratch row [s scratch_row_bytes, (s + 1) scratch_row_bytes).  max_row_bytes: the longest row of the table
 *   (sizes the grid).  Returns -1 before any launch for: a null or misaligned table / parent / own_pos / scratch (scratch: 16 bytes);
 *   n_entries or S outside 1 ... 65535; scratch_row_bytes or max_row_bytes < 16, no multiple of 16, or max_row_bytes >
 *   scratch_row_bytes; back other than 0 or 1. */
#define EVO_BEAM_MAX_WIDTH 8
#define EVO_GATHER_FIELDS 6
int evo_beam_select_f32(const void* logits, int64_t logits_f32, int64_t ld, const void* allow, const void* stop_mask,
                        const uint8_t* group_active, float* cum, uint8_t* ended, int64_t* length, int64_t* ids, int64_t* parent,
                        int32_t* hist_parent, int64_t* hist_ids, float* hist_cum, int64_t hist_len, int64_t* step, int64_t t,
                        int64_t W, int64_t S, int64_t V, void* stream);
int evo_gather_rows(const int64_t* table, int64_t n_entries, const int64_t* parent, const int64_t* own_pos, void* scratch,
                    int64_t scratch_row_bytes, int64_t max_row_bytes, int64_t S, int64_t back, void* stream);

/* ---- row-invariant weight-streaming dense layers (added under ABI 20, no signature changed; csrc/gemv_inv.hip; no counterpart in the reference) -------
 * The dense launches of a decode step whose results must not depend on how many rows ride along.  For 1 <= M <= 64 every output element is
 * computed by ONE fixed sequence of operations that is a function of (N, K) alone -- launch form, partition of K, reduction order: row i of
 * an M-row call is bit for bit the M = 1 call on row i, whatever the other rows hold (NaN included).  fp32 accumulate, one rounding.
 *   evo_linear_rowinv_bf16:   y [M, N] = x [M, K] . w [N, K]^T (+ bias [N]) (+ residual [M, N], may alias y).  K % 256 == 0, N % 64 == 0.
 *       N >= 8192: one launch, a wave per 16-row n tile sums the whole K in k order; `ws` is not read.
 *       N <  8192: K is cut into s = min(8, K / 256, ceil(256 / g)) slices of whole 256-k units (g = N / 64 workgroup columns; N / 32 below
 *       N = 2048); the slices' fp32 partial sums go through `ws` (16-byte aligned, ws_bytes >= s M N 4; 8 M N 4 always suffices) and a
 *       second launch adds them in slice order, then bias, then residual.
 *   evo_mlp_gate_rowinv_bf16: a [M, I] = gelu(bf16(x . W1^T)) * bf16(x . W2^T), w12 = [W1; W2] ([2 I, K]; `grouped` != 0: in
 *       pack_gate_weights' row order), as evo_mlp_gate_small_m_bf16 computes it at 5-64 rows.  K % 256 == 0, I % 32 == 0.
 * Both return -1 for a shape outside the contract (and the linear entry for a missing or short workspace): there is no second form. */
int evo_linear_rowinv_bf16(const void* x, const void* w, const void* bias, const void* residual, void* y, int64_t M, int64_t N,
                           int64_t K, void* ws, int64_t ws_bytes, void* stream);
int evo_mlp_gate_rowinv_bf16(const void* x, const void* w12, void* a, int64_t M, int64_t I, int64_t K, int64_t grouped, void* stream);

/* ---- box-calibration probes (measurement infrastructure; no reference counterpart) -----------------------------------
 * Two FIXED kernels whose rates depend on the box (HBM, the clocks its power cap allows) and on nothing else in this library:
 * bench.py times them in the same process right before the headline so that a driver-timed number can be compared across
 * boxes and rounds.
 *   evo_probe_copy_f4:   dst[i] = src[i], 16 bytes per lane, grid-stride (nbytes % 16 == 0): the guide's "float4 copy".
 *   evo_probe_mfma_bf16: n_blocks workgroups of 4 waves (one per SIMD), each wave `iters` trips of 16 independent
 *                        v_mfma_f32_16x16x32_bf16 on register-resident pseudo-random bf16 operands (never zeros);
 *                        flop = n_blocks * 4 * iters * 16 * 16384.  out [n_blocks * 256] fp32 sink or NULL. */
int evo_probe_copy_f4(const void* src, void* dst, int64_t nbytes, void* stream);
int evo_probe_mfma_bf16(float* out, int64_t n_blocks, int64_t iters, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* EVO_MI355X_H */
