"""What the host forward (sh/model.py, sp.py, scoring.py, pool.py) may ask of its `ops` object: `Backend`, the base of
`evo_amd.ops.HipOps` (the product's only backend) and of the oracle-backed backends the CPU tests inject.

REQUIRED of every backend (the modal route of a forward uses nothing else):
    embed(ids, weight, validate=True)                        linear(x, w, b=None, mfma=False)
    rmsnorm(x, bias, scale, eps)                             linear_residual_(res, x, w, mfma=False, bias=None)
    norm_linear(x, scale, eps, w, b=None, mfma=False)        mlp_gate(x, w12, norm_scale=None, eps=0.0, w12g=None)
    hyena_prefill(z, fir_w, fir_b, poles, residues, dskip, n_heads, z_halo=None, s0=None, want_state=False, seg_len=None, mask=None)
    hyena_decode_fused(x, norm_scale, eps, proj_w, proj_b, fir_state, iir_state, fir_w, fir_b, poles, residues, dskip, n_heads)
    hyena_stage1(z, fir_w, fir_b, poles, n_heads, z_halo=None, seg_len=None)      (sequence parallelism)
    hyena_stage2(z, fir_w, fir_b, poles, residues, dskip, n_heads, stage1, z_halo=None, s0=None)
    rope_(qkv, cos, sin, q_scale=1.0)                        attention(q, k, v, q_pos0, prescaled=False)
    attention_decode(q, k, v, pos=None, n_splits=None, prescaled=False)
    logprob_entropy(logits, target, want_logprob=True, want_entropy=False)
  (`q_scale` / `prescaled` differ from 1.0 / False only for a backend whose `attn_prescale` is set.)
ROUTING FLAGS are class attributes, all off: a backend that sets one provides that route's kernels.  OPTIONAL kernels are asked for with
`supports(*names)`, never by probing for a method name.  The PURE HOST FUNCTIONS are needed whatever the backend is.
"""
from __future__ import annotations

import math

import torch


class Backend:
    name = "backend"

    # ---- routing flags the host reads ------------------------------------------------------------------------------------------------
    hyena_mfma = False          # parallel Hyena calls take the single-pass matrix-core operator ...
    hyena_ct_flag = False       # ... on channel-major z^T (both set: the channel-major route; needs "hyena_ct")
    fuse_norm = False           # RMSNorm passes ride in the epilogues of the dense layers around them (needs "norm_fold")
    mlp_gate_fused = False      # the gated MLP's first half as one launch on the regrouped l1 | l2 (pack_gate_weights)
    attn_prescale = False       # rope_ folds attn_q_scale(hd) into q, the attention kernels take scores as exponents
    hyena_tail_split = False    # T = 512 k + 1 scoring: the one tail token through the fused single-token launch
    hyena_table_guard = True    # Hyena layers whose filter the operand tables cannot hold take the modal route
    timer = None                # a KernelTimer while bench.py times launches (the captured decode step is then off)
    attn_group_rows = 4         # batch rows per workgroup tile of the grouped decode attention (DecodePool's prefix_streams counter)

    # ---- optional kernel groups: the methods each one stands for ---------------------------------------------------------------------
    OPTIONAL = {
        "hyena_ct": ("hyena_ct", "rmsnorm_rows", "linear_t", "yblk_empty", "linear_residual_yblk_", "zt_shape_ok"),
        "norm_fold": ("nf_shape_ok", "zt_stream_rows_ok", "linear_rs", "linear_t_rs", "mlp_gate_rs", "linear_residual_stats_", "linear_residual_yblk_stats_"),
        "unembed_logprob": ("unembed_logprob", "unembed_logprob_ok"),
        "kv_fp8": ("kv_quant_fp8", "rope_append_decode_fp8", "attention_decode_fp8"),     # the FP8 KV cache (InferenceParams.kv_dtype == "fp8")
        # FP8 weights for the single-token step at 1 .. W8_ROWS rows (InferenceParams.weight_dtype == "fp8"): w_quant_fp8(w) -> Fp8Weight; the others
        # are linear / linear_residual_ / norm_linear / hyena_decode_fused / mlp_gate with the record in place of the weight(s)
        "w_fp8": ("w_quant_fp8", "linear_w8", "linear_residual_w8_", "norm_linear_w8", "hyena_decode_fused_w8", "mlp_gate_w8"),
        "kv_paged": ("rope_append_decode_paged", "attention_decode_paged"),               # the paged KV cache (InferenceParams.kv_layout == "paged")
        # the batch-invariant single-token step (InferenceParams.batch_invariant): dense launches whose rows do not see how many ride along --
        # linear_rowinv(x, w, b=None), linear_residual_rowinv_(res, x, w, bias=None), mlp_gate_rowinv(x_normed, w12, w12g=None); that step
        # also calls hyena_step(z_t, fir_state, iir_state, fir_w, fir_b, poles, residues, dskip, n_heads) where the default one is fused
        "row_invariant": ("linear_rowinv", "linear_residual_rowinv_", "mlp_gate_rowinv"),
        # beam search (DecodePool.beam_search): the step's selection, and the copy that moves a slot's records to the slot that continues it
        "beam": ("beam_select", "gather_rows"),
        # k-mer repeat control (DecodePool.generate(repeat=...)): the launch in front of the job-control sampler launch
        "repeat": ("repeat_rows",),
    }   # (single kernels go by their own name: rope_append_decode, unembed_profile, attention_prefix, attention_prefix_vt, attention_decode_prefix)

    def supports(self, *names: str) -> bool:
        """Does this backend provide every method of the named optional groups (a name outside OPTIONAL: the method of that name)?"""
        return all(hasattr(self, m) for n in names for m in self.OPTIONAL.get(n, (n,)))

    @staticmethod
    def adopt(ops):
        """`ops` itself if it is a Backend (or None); any other object -- a duck-typed stand-in written before this contract -- wrapped."""
        return ops if ops is None or isinstance(ops, Backend) else _Adopted(ops)

    # ---- pure host functions ---------------------------------------------------------------------------------------------------------
    DECODE_ROWS = 8     # batches this small take the fused single-token launches (csrc/gemv.hip; 5-8 rows at a width of 4096 only)
    W8_ROWS = 8         # batch rows the "w_fp8" launches serve (a routing fact, declared, not probed for: HipOps serves 64)
    YBLK = 128          # rows per block of the blocked y layout (csrc/hyena_ct.hip)
    ZT_ALIGN = 64       # positions a batch row of z^T is padded to (% 8 == 0: 16-byte loads; 64 = whole cache lines -- tools/hc_bench.py A/B)

    @staticmethod
    def fused_rows_ok(M: int, K: int) -> bool:
        """This many rows of width K fit the fused single-token launches (csrc/gemv.hip: norm + dense layer (+ gate / Hyena step) in one)."""
        return 1 <= M <= 4 or (M <= Backend.DECODE_ROWS and K == 4096)

    @staticmethod
    def zt_layout(B: int, T: int):
        """(Tm, Tp, Mp, r): where batch row b / token t of a [B, T] batch sits in z^T -- a pure function of the sizes.
        Position b * Tp + t for t < Tm (the MAIN area: Mp = B Tp rounded up to the dense layer's 256-row tile positions), and for the
        r = T - Tm last tokens of a row position Mp + 8 b + (t - Tm) (the TAIL block, one more block of 256 positions behind the main area).
        Plain form: r = 0, Tm = T, Tp = T rounded up to ZT_ALIGN.  Tail form: T = 512 k + r with 1 <= r <= 8 (the bench shapes: a BOS token in
        front of 2^k nucleotides) -- rows of 512 k positions need no padding and B * 512 k is a whole number of tiles, where the padded rows
        cost the persistent dense layer one more round (+2.5 ... 4 % per projection, profiles/r04_hyena_ct_notes.txt section 3); the B r <= 16
        tail tokens go through the weight-streaming kernel, as the BOS sliver of every other dense layer does (_tail_rows)."""
        al = Backend.ZT_ALIGN
        Tp = (T + al - 1) // al * al
        Mp = (B * Tp + 255) // 256 * 256
        r = T % 512
        Tm = T - r
        if 1 <= r <= 8 and Tm >= 512 and B * r <= 16 and Tm % al == 0 and (B * Tm + 255) // 256 * 256 < Mp:
            return Tm, Tm, (B * Tm + 255) // 256 * 256, r
        return T, Tp, Mp, 0

    @staticmethod
    def zt_geometry(B: int, T: int):
        """(Tp, Mp) of zt_layout: the row pitch and the number of positions of the main area."""
        _, Tp, Mp, _ = Backend.zt_layout(B, T)
        return Tp, Mp

    @staticmethod
    def zt_positions(B: int, T: int, b: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
        """Position in z^T of (batch row b, token t), elementwise (zt_layout)."""
        Tm, Tp, Mp, r = Backend.zt_layout(B, T)
        return torch.where(t < Tm, b * Tp + t, Mp + 8 * b + (t - Tm))

    @staticmethod
    def zt_rows(zt: torch.Tensor, B: int, T: int, t0: int, n: int) -> torch.Tensor:
        """Steps t0 .. t0 + n - 1 of every batch row of a channel-major z^T [blocks, 3 D, 256] as token-major [B, n, 3 D] (reference
        column order)."""
        bb = torch.arange(B, device=zt.device)[:, None].expand(B, n)
        tt = torch.arange(t0, t0 + n, device=zt.device)[None, :].expand(B, n)
        pos = Backend.zt_positions(B, T, bb, tt).reshape(-1)
        return zt[pos // 256, :, pos % 256].view(B, n, zt.shape[1])

    @staticmethod
    def zt_from_rows(z: torch.Tensor, B: int, T: int, pad_value: float = 0.0) -> torch.Tensor:
        """The inverse for whole sequences (tests, tools): token-major z [B, T, C] -> z^T [blocks, C, 256], pad positions = pad_value."""
        Tm, Tp, Mp, r = Backend.zt_layout(B, T)
        C = z.shape[-1]
        P = Mp + (256 if r else 0)
        flat = torch.full((C, P), pad_value, dtype=z.dtype, device=z.device)
        flat[:, :B * Tp].view(C, B, Tp)[:, :, :Tm] = z[:, :Tm].permute(2, 0, 1)
        if r:
            flat[:, Mp:].view(C, 32, 8)[:, :B, :r] = z[:, Tm:].permute(2, 0, 1)
        return flat.view(C, P // 256, 256).permute(1, 0, 2).contiguous()

    @staticmethod
    def fold_norm_scale(w: torch.Tensor, g: torch.Tensor) -> torch.Tensor:
        """W diag(g) as a bf16 copy (fp32 product, one rounding): the weight the norm-consuming launches multiply the RAW stream by."""
        return (w.float() * g.float()[None, :]).to(torch.bfloat16).contiguous()

    @staticmethod
    def pack_gate_weights(w12: torch.Tensor) -> torch.Tensor:
        """[W1; W2] ([2 I, K]) -> the row order evo_mlp_gate_mfma_bf16 wants: blocks of 64 rows = rows 32 q .. 32 q + 31 of W1
        followed by the same rows of W2, so that an output tile of the dense layer holds z1 and z2 of the same gated columns."""
        I2, K = w12.shape
        I = I2 // 2
        if I % 32:
            raise ValueError(f"pack_gate_weights: inner size {I} is not a multiple of 32")
        return torch.stack([w12[:I].view(I // 32, 32, K), w12[I:].view(I // 32, 32, K)], 1).reshape(I2, K).contiguous()

    @staticmethod
    def attn_q_scale(hd: int) -> float:
        """softmax_scale * log2(e) for head dim hd: what `rope_(..., q_scale=)` folds into the queries when the attention runs `prescaled`."""
        return (1.0 / math.sqrt(hd)) * 1.4426950408889634


class _Adopted(Backend):
    """An ops object that is no Backend, adopted at the model's door (Backend.adopt): its own attributes win, what it lacks reads as the
    contract's default, and a neutral q_scale / prescaled is not passed on to its rotary / attention methods (it may predate them)."""

    def __init__(self, ops):
        object.__setattr__(self, "_ops", ops)

    def __getattribute__(self, name):
        ops = object.__getattribute__(self, "_ops")
        if not hasattr(ops, name):
            return object.__getattribute__(self, name)
        attr = getattr(ops, name)
        if not name.startswith(("rope_", "attention")):
            return attr
        return lambda *a, **kw: attr(*a, **{k: v for k, v in kw.items() if (k, v) not in (("q_scale", 1.0), ("prescaled", False))})

    def __setattr__(self, name, value):
        setattr(self._ops, name, value)
