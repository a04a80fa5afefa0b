"""ctypes binding of libevo_mi355x.so (include/evo_mi355x.h) and the op set the StripedHyena host code calls.

`HipOps` is the ONLY compute backend the product ships: it raises if the shared library cannot be
loaded or a tensor is not on a ROCm device -- there is no CPU / eager fallback.  Every kernel of a scoring or generation
step -- the dense layers included (csrc/gemm.hip, csrc/gemv.hip) -- is a hand-written gfx950 kernel reached through the C ABI with
raw device pointers and the caller's current stream; hipBLASLt (through `torch.addmm`) serves only shapes no 7B layer has and the
in-process A/B knob `all_gemm_mfma = False`.
"""
from __future__ import annotations

import ctypes
import math
import os
import threading
from typing import Optional, Tuple

import torch

from . import _build
from .backend import Backend

_c = ctypes
_PTR = _c.c_void_p
_I64 = _c.c_int64
_F32 = _c.c_float

_SIGNATURES = {
    "evo_abi_version": ([], _c.c_int),
    "evo_embed_bf16": ([_PTR, _PTR, _PTR, _I64, _I64, _I64, _PTR, _PTR], _c.c_int),
    "evo_rmsnorm_bf16": ([_PTR, _PTR, _PTR, _PTR, _I64, _I64, _F32, _PTR], _c.c_int),
    "evo_hyena_seg_state": ([_PTR, _PTR, _PTR, _PTR, _PTR, _PTR, _PTR, _I64, _I64, _I64, _I64, _I64, _PTR], _c.c_int),
    "evo_hyena_carry_scan": ([_PTR, _PTR, _PTR, _PTR, _I64, _I64, _I64, _I64, _PTR], _c.c_int),
    "evo_hyena_carry_add": ([_PTR, _PTR, _PTR, _I64, _I64, _I64, _I64, _PTR], _c.c_int),
    "evo_hyena_apply": ([_PTR] * 10 + [_I64] * 5 + [_PTR], _c.c_int),
    "evo_hyena_step": ([_PTR] * 9 + [_I64] * 3 + [_PTR], _c.c_int),
    "evo_rope_qk_bf16": ([_PTR, _PTR, _PTR, _I64, _I64, _I64, _I64, _F32, _PTR], _c.c_int),
    "evo_attn_fwd_causal_bf16": ([_PTR] * 4 + [_I64] * 14 + [_F32, _PTR, _PTR], _c.c_int),
    "evo_attn_fwd_prefix_bf16": ([_PTR] * 6 + [_I64] * 16 + [_F32, _PTR, _PTR], _c.c_int),
    "evo_attn_prefix_vt_bf16": ([_PTR] * 2 + [_I64] * 5 + [_PTR], _c.c_int),
    "evo_attn_decode_bf16": ([_PTR] * 4 + [_I64] * 11 + [_PTR] * 3 + [_I64, _F32, _PTR], _c.c_int),
    "evo_linear_small_m_bf16": ([_PTR] * 5 + [_I64] * 3 + [_PTR, _I64, _PTR], _c.c_int),
    "evo_linear_mfma_bf16": ([_PTR] * 5 + [_I64] * 3 + [_PTR], _c.c_int),
    "evo_mlp_gate_mfma_bf16": ([_PTR] * 3 + [_I64] * 3 + [_PTR], _c.c_int),
    "evo_hyena_ct": ([_PTR] * 9 + [_I64] * 13 + [_PTR], _c.c_int),
    "evo_linear_t_mfma_bf16": ([_PTR] * 4 + [_I64] * 3 + [_PTR], _c.c_int),
    "evo_rmsnorm_rows_bf16": ([_PTR, _PTR, _PTR, _PTR, _I64, _I64, _F32, _I64, _I64, _I64, _I64, _PTR], _c.c_int),
    "evo_linear_xblk_mfma_bf16": ([_PTR] * 5 + [_I64] * 3 + [_PTR], _c.c_int),
    "evo_linear_mfma_nf_bf16": ([_PTR] * 7 + [_I64] * 4 + [_PTR], _c.c_int),
    "evo_linear_xblk_mfma_nf_bf16": ([_PTR] * 6 + [_I64] * 4 + [_PTR], _c.c_int),
    "evo_mlp_gate_mfma_nf_bf16": ([_PTR] * 4 + [_I64] * 3 + [_PTR], _c.c_int),
    "evo_linear_t_mfma_nf_bf16": ([_PTR] * 5 + [_I64] * 6 + [_PTR], _c.c_int),
    "evo_rms_finalize_f32": ([_PTR, _I64, _I64, _PTR, _I64, _I64, _I64, _F32, _PTR, _PTR], _c.c_int),
    "evo_probe_copy_f4": ([_PTR, _PTR, _I64, _PTR], _c.c_int),
    "evo_probe_mfma_bf16": ([_PTR, _I64, _I64, _PTR], _c.c_int),
    "evo_mlp_gate_small_m_bf16": ([_PTR] * 3 + [_I64] * 4 + [_PTR], _c.c_int),
    "evo_norm_linear_small_m_bf16": ([_PTR] * 5 + [_I64] * 3 + [_c.c_float, _PTR], _c.c_int),
    "evo_norm_mlp_gate_small_m_bf16": ([_PTR] * 4 + [_I64] * 3 + [_c.c_float, _I64, _PTR], _c.c_int),
    "evo_hyena_decode_fused_small_m": ([_PTR] * 12 + [_I64] * 3 + [_c.c_float, _PTR], _c.c_int),
    "evo_gelu_gate_bf16": ([_PTR, _PTR, _I64, _I64, _PTR], _c.c_int),
    "evo_logprob_entropy": ([_PTR, _I64, _PTR, _PTR, _PTR, _I64, _I64, _PTR], _c.c_int),
    "evo_unembed_logprob_bf16": ([_PTR] * 5 + [_I64] * 3 + [_PTR], _c.c_int),
    "evo_unembed_profile_bf16": ([_PTR] * 3 + [_c.POINTER(_c.c_int32), _I64] + [_PTR] * 3 + [_I64] * 3 + [_PTR], _c.c_int),
    "evo_rope_append_decode_bf16": ([_PTR] * 4 + [_F32] + [_I64] * 7 + [_F32, _PTR], _c.c_int),
    "evo_pool_rows_bf16": ([_PTR, _I64, _I64, _I64, _PTR, _I64, _PTR, _F32, _I64, _I64, _PTR, _PTR, _PTR], _c.c_int),
    "evo_attn_decode_prefix_bf16": ([_PTR] * 4 + [_I64] * 11 + [_PTR] * 3 + [_I64] * 8 + [_PTR] * 4 + [_I64, _I64, _F32, _PTR], _c.c_int),
    "evo_rope_append_decode_at_bf16": ([_PTR] * 4 + [_F32] + [_I64] * 7 + [_F32, _PTR, _PTR], _c.c_int),
    "evo_hyena_state_at_zt": ([_PTR] * 8 + [_I64] * 8 + [_PTR], _c.c_int),
    "evo_sample_rows_f32": ([_PTR, _I64, _I64, _PTR, _PTR, _PTR, _PTR, _c.c_uint64] + [_PTR] * 7 + [_I64] * 3 + [_PTR], _c.c_int),
    "evo_sample_rows_ctl_f32": ([_PTR, _I64, _I64, _PTR, _PTR, _PTR, _PTR, _c.c_uint64] + [_PTR] * 8 + [_I64] + [_PTR] * 4 + [_I64, _I64, _PTR, _PTR,
                                                                                                                         _I64, _I64, _PTR], _c.c_int),
    "evo_sample_rows_dfa_f32": ([_PTR, _I64, _I64, _PTR, _PTR, _PTR, _PTR, _c.c_uint64] + [_PTR] * 8 + [_I64] + [_PTR] * 4 + [_I64, _I64, _PTR, _PTR,
                                                                                                                         _PTR, _I64, _PTR, _I64,
                                                                                                                         _PTR, _PTR, _I64, _I64,
                                                                                                                         _PTR], _c.c_int),
    "evo_kv_quant_fp8": ([_PTR] * 4 + [_I64] * 18 + [_PTR], _c.c_int),
    "evo_rope_append_decode_fp8": ([_PTR] * 5 + [_F32] + [_I64] * 10 + [_F32, _PTR], _c.c_int),
    "evo_attn_decode_fp8": ([_PTR] * 4 + [_I64] * 12 + [_PTR] * 3 + [_I64, _F32, _PTR], _c.c_int),
    "evo_w_quant_fp8": ([_PTR] * 3 + [_I64] * 2 + [_PTR], _c.c_int),
    "evo_linear_small_m_w8": ([_PTR] * 6 + [_I64] * 3 + [_PTR, _I64, _PTR], _c.c_int),
    "evo_norm_linear_small_m_w8": ([_PTR] * 6 + [_I64] * 3 + [_F32, _PTR], _c.c_int),
    "evo_hyena_decode_fused_small_m_w8": ([_PTR] * 13 + [_I64] * 3 + [_F32, _PTR], _c.c_int),
    "evo_mlp_gate_small_m_w8": ([_PTR] * 4 + [_I64] * 4 + [_PTR], _c.c_int),
    "evo_norm_mlp_gate_small_m_w8": ([_PTR] * 5 + [_I64] * 3 + [_F32, _I64, _PTR], _c.c_int),
    "evo_linear_skinny_w8": ([_PTR] * 6 + [_I64] * 3 + [_PTR, _I64, _PTR], _c.c_int),
    "evo_mlp_gate_skinny_w8": ([_PTR] * 4 + [_I64] * 4 + [_PTR], _c.c_int),
    "evo_rope_append_decode_paged_bf16": ([_PTR] * 5 + [_F32] + [_I64] * 10 + [_F32, _PTR], _c.c_int),
    "evo_attn_decode_paged_bf16": ([_PTR] * 4 + [_I64] * 11 + [_PTR] * 3 + [_I64, _F32, _PTR], _c.c_int),
    "evo_beam_select_f32": ([_PTR, _I64, _I64] + [_PTR] * 11 + [_I64, _PTR] + [_I64] * 4 + [_PTR], _c.c_int),
    "evo_gather_rows": ([_PTR, _I64, _PTR, _PTR, _PTR] + [_I64] * 4 + [_PTR], _c.c_int),
    "evo_linear_rowinv_bf16": ([_PTR] * 5 + [_I64] * 3 + [_PTR, _I64, _PTR], _c.c_int),
    "evo_mlp_gate_rowinv_bf16": ([_PTR] * 3 + [_I64] * 4 + [_PTR], _c.c_int),
    "evo_repeat_rows_f32": ([_PTR, _I64, _I64] + [_PTR] * 8 + [_I64] + [_PTR] * 4 + [_I64] * 5 + [_PTR], _c.c_int),
}

_LIB = None
ABI_VERSION = 20        # must equal EVO_ABI_VERSION in include/evo_mi355x.h (bumped on every signature change)
ATTN_GROUP_ROWS = 8     # must equal EVO_ATTN_GROUP_ROWS there: batch rows per workgroup tile of attn_decode_group_kernel (the decode pool's
                        # `prefix_streams` counter is computed from it on the host)


HYENA_RAGGED_SEG = 256  # must equal EVO_HYENA_RAGGED_SEG there: steps per time segment of evo_hyena_state_at_zt (csrc/hyena_ragged.hip)


class EvoLibraryError(RuntimeError):
    pass


def load_library(build_if_missing: bool = True) -> ctypes.CDLL:
    """Load libevo_mi355x.so and type every entry point.  Raises EvoLibraryError when it is absent and
    cannot be built -- the product path never degrades to a non-HIP implementation."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = _build.lib_path()
    if (not path.exists() or (_build.is_stale() and os.environ.get("EVO_AMD_NO_REBUILD") != "1")) and build_if_missing:
        try:
            _build.build()
        except Exception as e:  # noqa: BLE001
            if not path.exists():
                raise EvoLibraryError(f"libevo_mi355x.so is missing and could not be built: {e}") from e
            import warnings                                  # a stale binary is usable only if its ABI still matches
            warnings.warn(f"{path} is older than its sources and the rebuild failed ({e}); loading the stale library "
                          f"(its ABI version is checked below)")
    if not path.exists():
        raise EvoLibraryError(f"{path} not found; run `python -c 'import __graft_entry__ as g; g.build()'`")
    lib = ctypes.CDLL(str(path))
    for name, (argtypes, restype) in _SIGNATURES.items():
        fn = getattr(lib, name, None)
        if fn is None:
            raise EvoLibraryError(f"{path} does not export {name}")
        fn.argtypes = argtypes
        fn.restype = restype
    got = lib.evo_abi_version()
    if got != ABI_VERSION:
        raise EvoLibraryError(f"{path} reports ABI version {got}, this binding needs {ABI_VERSION}: the library was built "
                              f"from other sources -- rebuild it (python -m evo_amd._build)")
    _LIB = lib
    return lib


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _check(code: int, name: str):
    if code != 0:
        raise RuntimeError(f"{name} failed with hipError/arg code {code}")


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def pick_segment_length(B: int, T: int, H: int, target_waves: int = 4096) -> int:
    """Time-segment length C of the Hyena kernels: enough (b, head, segment) waves to fill 256 CUs,
    power of two in [64, 1024]."""
    c = 1024
    while c > 64 and B * H * ((T + c - 1) // c) < target_waves:
        c //= 2
    return c


class KernelTimer:
    """HIP-event timing of individual launches ON THE STREAM THEY ARE LAUNCHED ON (torch's current stream).
    bench.py turns it on for the timed region to get per-kernel average durations for the roofline line."""

    def __init__(self):
        self.pairs = {}

    class _Span:
        def __init__(self, timer, name):
            self.timer, self.name = timer, name

        def __enter__(self):
            self.a = torch.cuda.Event(enable_timing=True)
            self.b = torch.cuda.Event(enable_timing=True)
            self.a.record()

        def __exit__(self, *exc):
            self.b.record()
            self.timer.pairs.setdefault(self.name, []).append((self.a, self.b))

    def span(self, name):
        return KernelTimer._Span(self, name)

    def summary(self):
        """{name: (launches, mean_ms)} -- call after a device synchronize."""
        return {k: (len(v), sum(a.elapsed_time(b) for a, b in v) / len(v)) for k, v in self.pairs.items()}


class _NoSpan:
    def __enter__(self):
        return None

    def __exit__(self, *exc):
        return False


_NOSPAN = _NoSpan()


class HipOps(Backend):
    """The gfx950 op set (the contract: evo_amd/backend.py).  All tensors must live on the same ROCm device."""

    name = "hip-gfx950"
    W8_ROWS = 64        # the FP8-weight launches serve 1-8 rows (csrc/gemv_fp8.hip) and 9-64 rows (csrc/skinny_fp8.hip)

    def __init__(self):
        self.lib = load_library()
        if not torch.cuda.is_available():
            raise EvoLibraryError("HipOps needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.seg_len_override = int(os.environ.get("EVO_AMD_SEG_LEN", "0"))
        # Routing (round 4): every prefill dense layer runs on the hand-written persistent kernel of csrc/gemm.hip -- no vendor GEMM in
        # a scoring step.  The attributes below are in-process A/B knobs for bench.py's legs and the tests (no environment switches):
        self.attn_gemm_mfma = True
        # prefill attention on the 64-rows-per-wave kernel of round 5 (csrc/attn_w64.hip); False: the 8-wave kernel of rounds 2-4 (bench A/B leg)
        self.attn_w64 = True
        # round 5: the RMSNorm passes of prefill-sized batches ride in the epilogues of the dense layers around them (csrc/gemm.hip, NF;
        # False = the separate rmsnorm launches: bench.py's A/B leg, the routing test)
        self.fuse_norm = True
        self.attn_prescale = True         # the model folds softmax_scale * log2(e) into the rotary kernel's one rounding of q; attention kernels take scores as exponents (csrc/attn_w64.hip PRE)
        # round 6: T = 512 k + 1 scoring batches (a BOS token in front of 2^k nucleotides) run the 512 k main tokens of every row through hyena_ct in
        # whole tiles and the one token behind them through the fused single-token launch, from the operator's end state; False: the ragged last
        # tile (one valid step at a full tile's issue time) inside the operator, the tail tokens' projections through the weight-streaming launch
        self.hyena_tail_split = True
        # round 6: the gated MLP's first half at 5-64 rows as ONE MFMA weight-streaming launch (False: dot2 launch up to 8 rows with a norm, dense layer + gate kernel above)
        self.gate_small_m_mfma = True
        self.hyena_table_guard = True     # Hyena layers whose filter the bf16 hi / lo operand tables cannot hold run the modal kernels (hyena_tables.table_precision)
        # all_gemm_mfma = False puts the plain dense layers (l3, the unembedding of model(ids)) back on hipBLASLt through torch.addmm:
        # the library is 1-3 % faster on l3's shape (K = 11,008; profiles/r03_gemm_notes.txt) -- bench.py times that leg beside the headline
        self.all_gemm_mfma = True
        # the gated MLP's first half as ONE launch of the dense layer with GELU * gate in its epilogue; False: dense layer + gate kernel
        self.mlp_gate_fused = True
        self.timer: Optional[KernelTimer] = None
        self.validate_ids = os.environ.get("EVO_AMD_VALIDATE_IDS", "1") != "0"   # one 4-byte D2H read per forward
        # the single-pass matrix-core Hyena operator on CHANNEL-MAJOR z^T (csrc/hyena_ct.hip: the projection launched with swapped
        # operands, no input window in LDS); False: the modal three-launch kernels (the tests' yardstick, padding masks, tiny inputs)
        self.hyena_mfma = True
        self.hyena_ct_flag = True
        self._xpad = threading.local()  # per thread: the zero-initialised padded input of the swapped-operand projection (_xpad_buffer), and the split-K workspaces of the 9-64-row FP8 launches (_skinny_w8_ws)
        self.last_hyena_io = {}

    def _t(self, name):
        return self.timer.span(name) if self.timer is not None else _NOSPAN

    # ---- plumbing -------------------------------------------------------------------------------
    PTR_ALIGN = 16      # bytes: the alignment include/evo_mi355x.h ("Conventions") asks of bf16 / f32 / c64 tensor data (16-byte vector loads / stores)

    @staticmethod
    def _align_of(dtype) -> int:
        """Bytes of alignment the header asks of an operand of this dtype: 16 for floating-point data, the element's own size for the
        integer vectors (ids, targets, positions, ranges: read one element at a time -- the model passes slices such as ids[b0:b0 + nb])."""
        return HipOps.PTR_ALIGN if (dtype.is_floating_point or dtype.is_complex) else torch.empty(0, dtype=dtype).element_size()

    @staticmethod
    def _check_address(addr: int, what: str, align: int = 16) -> None:
        """Raises when a device address breaks the header's alignment rule: a misaligned view fails here instead of reaching a kernel."""
        if addr % align:
            raise RuntimeError(f"{what}: address 0x{addr:x} is not {align}-byte aligned (include/evo_mi355x.h, Conventions)")

    @staticmethod
    def _need(t: torch.Tensor, dtype, what: str):
        if not t.is_cuda:
            raise RuntimeError(f"{what}: tensor is on {t.device}; the HIP path has no CPU fallback")
        if t.dtype != dtype:
            raise RuntimeError(f"{what}: expected {dtype}, got {t.dtype}")
        if not t.is_contiguous():
            raise RuntimeError(f"{what}: tensor must be contiguous")
        HipOps._check_address(t.data_ptr(), what, HipOps._align_of(dtype))

    @staticmethod
    def _need_strided(op: str, dims: Optional[int] = None, **operands) -> None:
        """The attention launches' q / k / v operands (strided views welcome): ROCm bf16, dense last dim, 16-byte aligned, `dims`-d if given."""
        for nm, t in ((nm, t) for nm, t in operands.items() if t is not None):
            if not t.is_cuda or t.dtype != torch.bfloat16 or t.stride(-1) != 1 or (dims is not None and t.dim() != dims):
                raise RuntimeError(f"{op} {nm}: need a {'' if dims is None else f'{dims}-d '}ROCm bf16 tensor with a dense last dim")
            HipOps._check_address(t.data_ptr(), f"{op} {nm}")

    def _launch(self, span: str, name: str, *args) -> None:
        """One launch of entry point `name` on the current stream, under the timer span `span`."""
        with self._t(span):
            _check(getattr(self.lib, name)(*args, _stream()), name)

    # ---- the dense layers' routing rules, each stated once ------------------------------------------
    TILE_ROWS = 256         # rows per tile of the persistent dense layer (csrc/gemm.hip GBM)
    SLIVER_ROWS = 16        # the most rows behind the last whole tile that count as a BOS sliver (the weight-streaming kernel's MFMA form: one m tile)
    TAIL_ROWS_FROM = 4096   # _tail_rows peels a sliver from this many rows on (below, one more row of tiles costs less than a second launch)

    @staticmethod
    def _bf16_ok(*tensors, scale=None) -> bool:
        """Every tensor is a contiguous bf16 device tensor -- what the hand-written launches ask of an operand -- and `scale` (a norm's
        scale vector), when given, contiguous bf16."""
        return (all(t.is_cuda and t.dtype == torch.bfloat16 and t.is_contiguous() for t in tensors)
                and (scale is None or (scale.dtype == torch.bfloat16 and scale.is_contiguous())))

    @staticmethod
    def _gemm_shape_ok(M: int, N: int, K: int, persistent: bool = True) -> bool:
        """The shape contract of csrc/gemm.hip for x [M, K] @ w [N, K]^T: whole 256-column tiles and 64-wide k steps; the PERSISTENT kernel
        also wants two k steps for its pipeline and both operands below 4 GiB (32-bit DMA offsets; outputs are addressed per tile)."""
        return (N % 256 == 0 and K % 64 == 0
                and (not persistent or (K >= 128 and M * K * 2 < 0xffffffff and N * K * 2 < 0xffffffff)))

    @staticmethod
    def _sliver_rows(M: int, limit: int = SLIVER_ROWS, floor: int = 0) -> int:
        """Rows of an M-row dense layer that go to the weight-streaming kernel: the 1 .. `limit` rows behind the last whole 256-row tile
        (none when there are more, or fewer than `floor` rows in all)."""
        r = M % HipOps.TILE_ROWS
        return r if M >= floor and 1 <= r <= limit else 0

    def _main_then_sliver(self, M: int, r: int, main, sliver) -> None:
        """The two launches of a dense layer of M rows whose last r are a sliver: `main(Mm)` for rows [0, Mm = M - r) -- whole tiles on the
        persistent kernel --, then `sliver(Mm)` for the rows behind them (r = 0: no second launch).  Dense layers are row-independent."""
        main(M - r)
        if r:
            sliver(M - r)

    # ---- dense layers (hipBLASLt via torch) --------------------------------------------------------
    @staticmethod
    def _tail_rows(x, w) -> int:
        """Rows to peel off a big dense layer: the BOS token makes M = B * (nt + 1) = 256 k + (1..16), and that last
        sliver costs a whole extra row of 256-row tiles (measured on hipBLASLt: +0.7 ... +4.7 % per GEMM at
        M = 65,544, +0.5 ... +3.7 % at 131,073).  Dense layers are row-independent, so the sliver goes through the
        weight-streaming kernel instead."""
        M, K = x.shape
        return HipOps._sliver_rows(M, floor=HipOps.TAIL_ROWS_FROM) if K % 32 == 0 and HipOps._bf16_ok(x, w) else 0

    def linear(self, x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor] = None, mfma: bool = False) -> torch.Tensor:
        """x [M,K] @ w[N,K]^T (+ b) -> [M,N] bf16.  M <= 16 (decode) takes the weight-streaming kernels; `mfma=True`
        (the attention block's projections) takes the hand-written MFMA kernel of csrc/gemm.hip when the shape allows
        (`attn_gemm_mfma` / `all_gemm_mfma` False route to hipBLASLt: bench.py's A/B legs)."""
        if self._use_small_m(x, w):
            return self._linear_small_m(x, w, b, None)
        y = torch.empty(x.shape[0], w.shape[0], dtype=x.dtype, device=x.device)
        self._linear_into(y, x, w, b, mfma)
        return y

    def _take_mfma(self, mfma: bool) -> bool:
        return self.all_gemm_mfma or (mfma and self.attn_gemm_mfma)

    def _linear_into(self, y, x, w, b, mfma, residual: bool = False) -> None:
        """y = x @ w^T (+ b) (+ y itself with `residual`; fp32 accumulate, one rounding): the main rows on the persistent kernel when
        routing and shape allow (hipBLASLt otherwise), the BOS sliver on the weight-streaming kernel."""
        def main(Mm):
            xm, ym = x[:Mm], y[:Mm]
            if self._take_mfma(mfma) and self.mfma_linear_ok(xm, w) and ym.is_contiguous():
                self.linear_mfma(xm, w, b, ym if residual else None, out=ym)     # (bias and residual in the dense layer's epilogue: one rounding)
                return
            with self._t("gemm"):
                if residual:
                    ym.addmm_(xm, w.t())
                elif b is not None:
                    torch.addmm(b, xm, w.t(), out=ym)
                else:
                    torch.mm(xm, w.t(), out=ym)
            if residual and b is not None:
                ym.add_(b)
        self._main_then_sliver(x.shape[0], self._tail_rows(x, w) if y.is_contiguous() else 0, main,
                               lambda Mm: self._linear_small_m(x[Mm:], w, b, y[Mm:] if residual else None, out=y[Mm:]))

    def linear_residual_(self, res: torch.Tensor, x: torch.Tensor, w: torch.Tensor, mfma: bool = False,
                         bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        """res += x @ w^T (+ bias) (fp32 accumulate, one rounding), in place.  `bias` is for the decode path, where the
        weight-streaming kernel adds it in the same pass."""
        if self._use_small_m(x, w) and res.is_contiguous():
            return self._linear_small_m(x, w, bias, res)
        self._linear_into(res, x, w, bias, mfma, residual=True)
        return res

    @staticmethod
    def _use_small_m(x, w):
        """The weight-streaming kernels (csrc/gemv.hip) serve every decode-sized batch: dot2 form up to M = 4 (and
        for K % 32 != 0 up to M = 8), MFMA form for 5 <= M <= 16 (tools/bench_gemv.py for the crossovers) and -- round 6 -- for
        17 <= M <= 64 with 2-4 m tiles per weight pass (the pooled decode step at 17-64 live slots ran the persistent 256 x 256 GEMM
        there: N / 256 of the 256 CUs busy, 80 % of a 32-slot step; profiles/r06_pool32_kernel_stats.txt)."""
        M, K = x.shape
        if not (1 <= M <= (64 if K % 32 == 0 else 16)):
            return False
        if K % 32 != 0 and not (M <= 4 or (M <= 8 and w.shape[0] <= 4096)):
            return False
        return HipOps._bf16_ok(x, w) and K % 8 == 0

    def _linear_small_m(self, x, w, b, res, out=None):
        M, K = x.shape
        N = w.shape[0]
        y = res if res is not None else (out if out is not None else torch.empty(M, N, dtype=torch.bfloat16, device=x.device))
        # 17-64 rows on a narrow layer (N < 8192): a workspace for the partial sums of the split over K (csrc/gemv.hip skinny_nw_kernel SPLITK)
        ws = torch.empty(8 * M * N, dtype=torch.float32, device=x.device) if (M > 16 and N < 8192 and K % 256 == 0 and N % 64 == 0) else None
        self._launch("gemv", "evo_linear_small_m_bf16", x.data_ptr(), w.data_ptr(), _ptr(b), _ptr(res), y.data_ptr(), M, N, K, _ptr(ws),
                     0 if ws is None else ws.numel() * 4)
        return y

    @staticmethod
    def mfma_linear_ok(x, w):
        # not the persistent contract: evo_linear_mfma_bf16 serves K = 64 and operands beyond 4 GiB with its tile-per-workgroup kernel
        # (csrc/gemm.hip); 8 rows or fewer belong to the weight-streaming kernels whatever the operands
        return HipOps._bf16_ok(x, w) and HipOps._gemm_shape_ok(x.shape[0], w.shape[0], x.shape[1], persistent=False) and x.shape[0] > 8

    def linear_mfma(self, x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor] = None,
                    residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Hand-written MFMA dense layer (csrc/gemm.hip): x [M,K] @ w[N,K]^T (+ b) (+ residual, in place) -> [M,N] (`out`, when given)."""
        self._need(x, torch.bfloat16, "linear_mfma x")
        self._need(w, torch.bfloat16, "linear_mfma w")
        M, K = x.shape
        N = w.shape[0]
        if residual is not None:
            self._need(residual, torch.bfloat16, "linear_mfma residual")
        y = residual if residual is not None else (out if out is not None else torch.empty(M, N, dtype=torch.bfloat16, device=x.device))
        self._launch("gemm_mfma", "evo_linear_mfma_bf16", x.data_ptr(), w.data_ptr(), _ptr(b), _ptr(residual), y.data_ptr(), M, N, K)
        return y

    # ---- kernels -------------------------------------------------------------------------------------
    def embed(self, ids: torch.Tensor, weight: torch.Tensor, validate: bool = True) -> torch.Tensor:
        """Row gather.  Ids outside [0, vocab) raise IndexError (the reference's F.embedding device-asserts): the
        kernel never indexes the table with them and raises a device flag, which is read back here -- except while a
        hipGraph is being captured (no host read is possible there; the decode loop's ids come from `sample`).  `validate=False`: the
        caller has checked the ids itself (a sequence-parallel rank checks ALL of them before its first collective)."""
        ids = ids.reshape(-1).to(torch.int64).contiguous()
        self._need(ids, torch.int64, "embed ids")
        self._need(weight, torch.bfloat16, "embed weight")
        V, D = weight.shape
        out = torch.empty(ids.numel(), D, dtype=torch.bfloat16, device=weight.device)
        # a fresh 4-byte flag per call (a cached one would be an inference tensor when first made under
        # torch.inference_mode and could not be reset outside it); none while a hipGraph is being captured
        flag = None if torch.cuda.is_current_stream_capturing() or not (self.validate_ids and validate) else \
            torch.zeros(1, dtype=torch.int32, device=weight.device)
        _check(self.lib.evo_embed_bf16(ids.data_ptr(), weight.data_ptr(), out.data_ptr(), ids.numel(), D, V,
                                       _ptr(flag), _stream()), "evo_embed_bf16")
        if flag is not None and int(flag.item()) != 0:
            raise IndexError(f"input_ids contain values outside [0, {V}) (embedding table has {V} rows)")
        return out

    def rmsnorm(self, x: torch.Tensor, bias: Optional[torch.Tensor], scale: torch.Tensor, eps: float) -> torch.Tensor:
        """out = scale * x / (rms(x) + eps); with `bias`, x is first updated in place (x += bias)."""
        self._need(x, torch.bfloat16, "rmsnorm x")
        self._need(scale, torch.bfloat16, "rmsnorm scale")
        if bias is not None:
            self._need(bias, torch.bfloat16, "rmsnorm bias")
        M, D = x.shape
        out = torch.empty_like(x)
        with self._t("rmsnorm_bias" if bias is not None else "rmsnorm"):
            _check(self.lib.evo_rmsnorm_bf16(x.data_ptr(), _ptr(bias), scale.data_ptr(), out.data_ptr(), M, D,
                                             float(eps), _stream()), "evo_rmsnorm_bf16")
        return out

    # ---- the channel-major (z^T) form of the Hyena block's input: csrc/hyena_ct.hip -------------------------------------------
    def zt_shape_ok(self, B: int, T: int, N: int, K: int) -> bool:
        _, _, Mp, r = self.zt_layout(B, T)
        P = Mp + (256 if r else 0)
        return self.hyena_ct_flag and B * T >= 256 and N % 384 == 0 and self._gemm_shape_ok(Mp, N, K) and P * N * 2 < 0xfffffff0

    def _xpad_buffer(self, B: int, T: int, D: int, device) -> torch.Tensor:
        """The cached [Mp + 16, D] bf16 workspace of rmsnorm_rows: ONE layout at a time (a scoring run keeps its shape; another (B, T)
        -- even one with the same number of rows -- replaces the buffer by a freshly zeroed one, so pad rows never hold another
        layout's activations), one instance PER THREAD (callers that drive one HipOps from several threads -- the virtual ranks of the
        sequence-parallel tests, a server's worker threads -- must not share it: launches of different threads are not ordered with each
        other) and per STREAM (a second stream would otherwise reuse it with no event ordering).  Pad rows are zero when the buffer is
        made and never written by rmsnorm_rows; what the projection computes from them lands in pad positions of z^T, which hyena_ct
        masks.  `release_workspaces()` drops it (a long-lived server between shapes)."""
        key = (B, T, D, str(device), torch.cuda.current_stream().cuda_stream if torch.cuda.is_available() else 0)
        cur = getattr(self._xpad, "entry", None)
        if cur is None or cur[0] != key:
            _, _, Mp, _ = self.zt_layout(B, T)
            cur = (key, torch.zeros(Mp + 16, D, dtype=torch.bfloat16, device=device))
            self._xpad.entry = cur
        return cur[1]

    def release_workspaces(self) -> None:
        """Frees this thread's cached rmsnorm_rows workspace (0.5 GB at 8 x 8,193, 1 GB at 1 x 131,073 for D = 4096) and the split-K
        workspaces of the 9-64-row FP8 launches (_skinny_w8_ws)."""
        self._xpad.entry = None
        self._xpad.w8_ws = None

    def rmsnorm_rows(self, x: torch.Tensor, scale: torch.Tensor, eps: float, B: int, T: int) -> torch.Tensor:
        """RMSNorm of x [B T, D] written in the row order of zt_layout: -> [Mp + 16, D], row b T + t at its z^T position for t < Tm, the
        B r tail tokens compactly at rows Mp + b r + (t - Tm) (the weight-streaming kernel's input).  The buffer is a cached workspace
        (_xpad_buffer: pad rows are zero and never written), valid until this thread's next call on this stream."""
        self._need(x, torch.bfloat16, "rmsnorm x")
        self._need(scale, torch.bfloat16, "rmsnorm scale")
        M, D = x.shape
        assert M == B * T
        Tm, Tp, Mp, r = self.zt_layout(B, T)
        out = self._xpad_buffer(B, T, D, x.device)
        with self._t("rmsnorm"):
            _check(self.lib.evo_rmsnorm_rows_bf16(x.data_ptr(), None, scale.data_ptr(), out.data_ptr(), M, D, float(eps), T, Tp, Tm, Mp,
                                                  _stream()), "evo_rmsnorm_rows_bf16")
        return out

    def linear_t(self, xp: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor], B: int, T: int, tail: bool = True) -> torch.Tensor:
        """z^T = (x @ w [N, K]^T + b)^T in blocks of 256 positions, [Mp / 256 (+ 1), N, 256] bf16, from rmsnorm_rows' buffer xp: the dense
        layer launched with swapped operands on the Mp main rows (csrc/gemm.hip, mode 3), the tail tokens (zt_layout) through the
        weight-streaming kernel into the tail block; w in the REFERENCE's row order (no regrouped copy).  `tail=False`: the main area
        only (the caller takes the tail tokens through the single-token launch: hyena_ct(main_only=True))."""
        self._need(xp, torch.bfloat16, "linear_t x")
        self._need(w, torch.bfloat16, "linear_t w")
        Tm, Tp, Mp, r = self.zt_layout(B, T)
        K = xp.shape[1]
        N = w.shape[0]
        assert xp.shape[0] >= Mp + B * r
        zt = torch.empty(Mp // 256 + (1 if r and tail else 0), N, 256, dtype=torch.bfloat16, device=xp.device)
        self._launch("gemm_zt", "evo_linear_t_mfma_bf16", xp.data_ptr(), w.data_ptr(), _ptr(b), zt.data_ptr(), Mp, N, K)
        if r and tail:
            self._zt_tail_fill(zt, self._linear_small_m(xp[Mp:Mp + B * r], w, b, None), B, r)
        return zt

    @staticmethod
    def _zt_tail_fill(zt: torch.Tensor, z_tail: torch.Tensor, B: int, r: int) -> None:
        """The tail block of z^T (zt_layout) from the tail tokens' projections z_tail [B r, N]: token j of batch row b at position Mp + 8 b + j."""
        N = zt.shape[1]
        zt[-1].zero_()                                                                    # (6 MB: the tail block's unused positions hold zeros, not whatever the allocator left)
        zt[-1].view(N, 32, 8)[:, :B, :r] = z_tail.view(B, r, N).permute(2, 0, 1)

    def hyena_ct(self, zt, B, T, fir_w, fir_b, table, n_heads, z_halo=None, s0=None, want_state=False, poles=None,
                 state_only=False, b_first=0, y_blk=None, y_row0=0, b_total=None, main_only=False):
        """The channel-stationary single-pass operator on CHANNEL-MAJOR z (csrc/hyena_ct.hip: evo_hyena_ct): zt [blocks, 3 D, 256] bf16 =
        linear_t's result (zt_layout of a [b_total, T] batch; b_total defaults to b_first + B); B batch rows of T tokens starting at
        batch row `b_first` of the tensor (a sub-range).  -> y [B,T,D] bf16 | (y, end state [B,D,8] complex64) with `want_state` | the end state alone with `state_only` (stage 1 of a
        sequence-parallel shard: nothing else is written).  `z_halo` [B, 2, 3 D] in the REFERENCE's column order, `s0` [B,D,8] complex:
        FIR history / modal state before the first token.  `y_blk` (from yblk_empty): the outputs go THERE, blocked, batch row b /
        token t as row y_row0 + b T + t -- the form the kernel stores fastest and linear_residual_yblk_ reads.
        `main_only` (tail form of zt_layout only): the operator walks the Tm = 512 k main tokens of every row -- whole tiles -- and leaves
        rows b T + Tm .. of y untouched; with `want_state` the state returned is the one after token Tm - 1: the caller finishes the r
        tail tokens with the single-token launch (hyena_decode_fused / hyena_step) from that state (StripedHyena._hyena_block; a ragged
        tile with one valid step costs the kernel a full tile's issue time: 8 of 136 tile steps at 8 x 8,193)."""
        self._need(zt, torch.bfloat16, "hyena z^T")
        assert zt.dim() == 3 and zt.shape[2] == 256
        D3, P = zt.shape[1], zt.shape[0] * 256
        D = D3 // 3
        Tm, Tp, Mp, r = self.zt_layout(b_first + B if b_total is None else b_total, T)
        assert D3 == 3 * D and (b_first + B) * Tp <= Mp
        if main_only:
            assert r > 0 and P in (Mp, Mp + 256) and z_halo is None and s0 is None and not state_only
        else:
            assert P == Mp + (256 if r else 0)
        T_run = Tm if main_only else T
        if table.dtype != torch.int32 or tuple(table.shape) != (D, 52, 64) or not table.is_contiguous() or not table.is_cuda:
            raise RuntimeError("hyena_ct: table must be the contiguous int32 [D, 52, 64] tensor of mfma_operand_table")
        for t, nm in ((fir_w, "fir_w"), (fir_b, "fir_b")):
            self._need(t, torch.bfloat16, "hyena " + nm)
        if z_halo is not None:
            self._need(z_halo, torch.bfloat16, "hyena z_halo")
            assert z_halo.shape == (B, 2, 3 * D)
        s0r = None
        if s0 is not None:
            s0r = torch.view_as_real(s0.to(torch.complex64).contiguous())
            assert s0r.shape == (B, D, 8, 2) and s0r.is_cuda
        s_fin = None
        if want_state or state_only:
            if poles is None:
                raise RuntimeError("hyena_ct: the end state needs the poles")
            self._need(poles, torch.float32, "hyena poles")
            assert tuple(poles.shape) == (D, 8, 2)
            s_fin = torch.empty(B, D, 8, 2, dtype=torch.float32, device=zt.device)
        yb_rows = 0
        if state_only:
            y = None
        elif y_blk is not None:
            self._need(y_blk, torch.bfloat16, "hyena y (blocked)")
            assert y_blk.dim() == 4 and tuple(y_blk.shape[1:]) == (D // 16, self.YBLK, 16)
            yb_rows = y_blk.shape[0] * self.YBLK
            assert 0 <= y_row0 and y_row0 + B * T <= yb_rows
            y = y_blk
        else:
            y = torch.empty(B, T, D, dtype=torch.bfloat16, device=zt.device)
        with self._t("hyena_mfma_state" if state_only else "hyena_mfma"):
            _check(self.lib.evo_hyena_ct(zt.data_ptr(), _ptr(z_halo), fir_w.data_ptr(), fir_b.data_ptr(), table.data_ptr(), _ptr(y),
                                         _ptr(s0r), _ptr(s_fin), _ptr(poles), B, T_run, D, n_heads, P, Tp, b_first * Tp,
                                         Tm if r and not main_only else 0, Mp + 8 * b_first, 1 if state_only else 0, yb_rows, y_row0,
                                         T if main_only else 0, _stream()),
                   "evo_hyena_ct")
        if state_only:
            return torch.view_as_complex(s_fin)
        self.last_hyena_io = {"mfma": B * T_run * 3 * D * 2 + B * T_run * D * 2}
        return (y, torch.view_as_complex(s_fin)) if want_state else y

    def hyena_state_at_zt(self, zt, B, T, lens, fir_w, fir_b, poles, n_heads):
        """Ragged batch (csrc/hyena_ragged.hip: evo_hyena_state_at_zt): the modal state after token lens[b] - 1 of every batch row, from a
        zero start, and the two steps of FIR history there -- what a cached prefill of row b ALONE would hand to decode.  zt [blocks, 3 D,
        256] bf16 in the plain form of zt_layout(B, T); lens [B] int64 (a device tensor is never read by the host; values outside [1, T]
        are clamped).  -> (state complex64 [B, D, 8], fir bf16 [B, 3 D, 2]).  Positions at and behind lens[b] may hold anything."""
        self._need(zt, torch.bfloat16, "hyena z^T")
        assert zt.dim() == 3 and zt.shape[2] == 256
        D3, P = zt.shape[1], zt.shape[0] * 256
        D = D3 // 3
        _, Tp, Mp, r = self.zt_layout(B, T)
        if r or P != Mp or D3 != 3 * D:
            raise RuntimeError("hyena_state_at_zt: z^T must be the plain form of zt_layout (no tail block)")
        for t, nm in ((fir_w, "fir_w"), (fir_b, "fir_b")):
            self._need(t, torch.bfloat16, "hyena " + nm)
        self._need(poles, torch.float32, "hyena poles")
        assert tuple(poles.shape) == (D, 8, 2)
        lens = torch.as_tensor(lens, dtype=torch.int64).to(zt.device).contiguous()
        assert tuple(lens.shape) == (B,)
        state = torch.empty(B, D, 8, 2, dtype=torch.float32, device=zt.device)
        fir = torch.empty(B, D3, 2, dtype=torch.bfloat16, device=zt.device)
        args = (zt.data_ptr(), lens.data_ptr(), fir_w.data_ptr(), fir_b.data_ptr(), poles.data_ptr(), state.data_ptr(), fir.data_ptr())
        need = self.lib.evo_hyena_state_at_zt(*args, None, 0, B, T, D, n_heads, P, Tp, 0, None)
        if need < 0:
            raise RuntimeError(f"evo_hyena_state_at_zt refused B = {B}, T = {T}, D = {D}, heads = {n_heads}")
        ws = torch.empty(need // 4, dtype=torch.float32, device=zt.device)
        self._launch("hyena_state_at", "evo_hyena_state_at_zt", *args, ws.data_ptr(), need, B, T, D, n_heads, P, Tp, 0)
        return torch.view_as_complex(state), fir

    def hyena_state_at(self, z, lens, fir_w, fir_b, poles, n_heads):
        """The same from TOKEN-major z [B, T, 3 D] (the modal routing: layers the table guard refuses, shapes zt_shape_ok refuses): z is laid
        out channel-major (a copy -- a rare path) with T rounded up to a whole number of 64 positions, and goes through the same kernel."""
        B, T, D3 = z.shape
        Tw = (T + self.ZT_ALIGN - 1) // self.ZT_ALIGN * self.ZT_ALIGN
        if Tw != T:
            z = torch.nn.functional.pad(z, (0, 0, 0, Tw - T))
        lens = torch.as_tensor(lens, dtype=torch.int64).to(z.device).clamp(1, T)
        return self.hyena_state_at_zt(self.zt_from_rows(z, B, Tw), B, Tw, lens, fir_w, fir_b, poles, n_heads)

    def hyena_prefill(self, z: torch.Tensor, fir_w: torch.Tensor, fir_b: torch.Tensor, poles: torch.Tensor,
                      residues: torch.Tensor, dskip: torch.Tensor, n_heads: int,
                      z_halo: Optional[torch.Tensor] = None, s0: Optional[torch.Tensor] = None,
                      want_state: bool = False, seg_len: Optional[int] = None,
                      mask: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
        """z [B,T,3D] bf16 -> y [B,T,D] bf16 (+ complex64 state [B,D,8] after the last token).  `mask` [B,T] (bool /
        uint8, 1 = token) is upstream's padding_mask: padded positions get a zero FIR output.  The three-launch MODAL form
        (csrc/hyena.hip: segment states, carry scan, apply) on token-major z: padding masks, inputs the single-pass kernel's
        contract excludes, and the yardstick the tests hold hyena_ct against."""
        if mask is not None:
            mask = mask.to(device=z.device, dtype=torch.uint8).contiguous()
            assert mask.shape == z.shape[:2]
        self._need(z, torch.bfloat16, "hyena z")
        B, T, D3 = z.shape
        D = D3 // 3
        for t, nm in ((fir_w, "fir_w"), (fir_b, "fir_b"), (dskip, "dskip")):
            self._need(t, torch.bfloat16, "hyena " + nm)
        self._need(poles, torch.float32, "hyena poles")
        self._need(residues, torch.float32, "hyena residues")
        if z_halo is not None:
            self._need(z_halo, torch.bfloat16, "hyena z_halo")
            assert z_halo.shape == (B, 2, D3)
        s0r = None
        if s0 is not None:
            s0r = torch.view_as_real(s0.to(torch.complex64).contiguous())
            assert s0r.shape == (B, D, 8, 2)
        agg, C = self._hyena_seg_state(z, z_halo, fir_w, fir_b, poles, mask, n_heads, seg_len)
        s_final = torch.empty(B, D, 8, 2, dtype=torch.float32, device=z.device) if want_state else None
        self._launch("hyena_carry_scan", "evo_hyena_carry_scan", agg.data_ptr(), poles.data_ptr(), _ptr(s0r), _ptr(s_final), B, T, D, C)
        y = self._hyena_apply(z, z_halo, fir_w, fir_b, poles, residues, dskip, agg, mask, n_heads, C)
        state = torch.view_as_complex(s_final) if want_state else None
        # bytes of the tensors each launch touched (bench.py prints them beside the algorithmic figure)
        self.last_hyena_io = {"seg_state": z.numel() * 2 * 2 // 3 + agg.numel() * 4,
                              "apply": z.numel() * 2 + y.numel() * 2 + agg.numel() * 4}
        return y, state

    def _hyena_seg_state(self, z, z_halo, fir_w, fir_b, poles, mask, n_heads, seg_len):
        """Launch 1 of the modal form: the segments' end states from a zero carry-in -> (agg [B, segments, D, 8, 2] fp32, segment length)."""
        B, T, D3 = z.shape
        C = seg_len or self.seg_len_override or pick_segment_length(B, T, n_heads)
        agg = torch.empty(B, (T + C - 1) // C, D3 // 3, 8, 2, dtype=torch.float32, device=z.device)
        self._launch("hyena_seg_state", "evo_hyena_seg_state", z.data_ptr(), _ptr(z_halo), fir_w.data_ptr(), fir_b.data_ptr(), poles.data_ptr(),
                     agg.data_ptr(), _ptr(mask), B, T, D3 // 3, n_heads, C)
        return agg, C

    def _hyena_apply(self, z, z_halo, fir_w, fir_b, poles, residues, dskip, agg, mask, n_heads, C):
        """Launch 3 of the modal form: y [B, T, D] from z and the segments' carried-in states `agg`."""
        B, T, D3 = z.shape
        y = torch.empty(B, T, D3 // 3, dtype=torch.bfloat16, device=z.device)
        self._launch("hyena_apply", "evo_hyena_apply", z.data_ptr(), _ptr(z_halo), fir_w.data_ptr(), fir_b.data_ptr(), poles.data_ptr(),
                     residues.data_ptr(), dskip.data_ptr(), agg.data_ptr(), y.data_ptr(), _ptr(mask), B, T, D3 // 3, n_heads, C)
        return y

    def yblk_empty(self, rows: int, D: int, device) -> torch.Tensor:
        """Uninitialised BLOCKED y for a [rows, D] matrix: [ceil(rows / 128), D / 16, 128, 16] bf16 (hyena_ct writes it, the output
        projection's dense layer reads it: linear_residual_yblk_)."""
        return torch.empty((rows + self.YBLK - 1) // self.YBLK, D // 16, self.YBLK, 16, dtype=torch.bfloat16, device=device)

    @staticmethod
    def yblk_to_rows(y_blk: torch.Tensor, rows: int) -> torch.Tensor:
        """Blocked y -> the row-major [rows, D] matrix it stands for (a copy; tests, and shapes the blocked dense layer does not take)."""
        nrb, G, R, c = y_blk.shape
        return y_blk.permute(0, 2, 1, 3).reshape(nrb * R, G * c)[:rows]

    def linear_residual_yblk_(self, res: torch.Tensor, y_blk: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        """res [M, N] += y @ w^T (+ bias, in the same epilogue: one rounding) with y given BLOCKED (hyena_ct's y_blk: [ceil(M / 128), K / 16, 128, 16]) -- the Hyena block's output
        projection on the hand-written dense layer (csrc/gemm.hip, X operand gathered from the blocked form); the last M % 256
        rows (the BOS sliver) go row-major through the weight-streaming kernel, as everywhere."""
        M, N = res.shape
        K = w.shape[1]
        assert y_blk.shape[0] * self.YBLK >= M and y_blk.shape[1] * 16 == K and res.is_contiguous()
        r = self._sliver_rows(M, limit=255)                  # (the blocked launch takes whole tiles only)
        if not (M > r and self._gemm_shape_ok(M - r, N, K) and self._bf16_ok(w)):
            return self.linear_residual_(res, self.yblk_to_rows(y_blk, M).contiguous(), w, bias=bias)
        self._main_then_sliver(M, r,
                               lambda Mf: self._launch("gemm_mfma", "evo_linear_xblk_mfma_bf16", y_blk.data_ptr(), w.data_ptr(), _ptr(bias),
                                                       res.data_ptr(), res.data_ptr(), Mf, N, K),
                               lambda Mf: self.linear_residual_(res[Mf:], self._yblk_tail_rows(y_blk, Mf, M), w, bias=bias))
        return res

    def _yblk_tail_rows(self, y_blk: torch.Tensor, Mf: int, M: int) -> torch.Tensor:
        """Rows Mf .. M - 1 (Mf a multiple of 256, at most 255 rows) of the matrix a blocked y stands for, gathered row-major."""
        return y_blk[Mf // self.YBLK:].permute(0, 2, 1, 3).reshape(-1, y_blk.shape[1] * 16)[:M - Mf].contiguous()

    # ---- RMSNorm folded into the dense layers around it (csrc/gemm.hip NF; include/evo_mi355x.h "RMSNorm folded ...") -----------------
    def nf_shape_ok(self, M: int, N: int, K: int) -> bool:
        """Shapes whose main rows the persistent dense layer takes with the norm folded in (sliver rows <= 16 or none)."""
        # (below 1,024 rows a forward is launch-bound -- four row tiles on 256 CUs -- and the fold would trade 63 small norm launches for 64 finalize launches)
        return self.fuse_norm and self.all_gemm_mfma and M >= 1024 and self._gemm_shape_ok(self._nf_main_rows(M), N, K)

    def _nf_main_rows(self, M: int) -> int:
        return M - self._sliver_rows(M)                      # (no floor of its own: nf_shape_ok asks for 1,024 rows)

    def rms_finalize(self, ss: Optional[torch.Tensor], x: torch.Tensor, M_main: int, eps: float) -> torch.Tensor:
        """rstd [M rounded up to 256] fp32 = 1 / (rms(x_m) + eps): rows < M_main from the dense layer's partial sums `ss`
        [strips, ld], the others from x itself (evo_rms_finalize_f32)."""
        M, D = x.shape
        rstd = torch.empty((M + 255) // 256 * 256, dtype=torch.float32, device=x.device)
        self._launch("rms_finalize", "evo_rms_finalize_f32", _ptr(ss), 0 if ss is None else ss.shape[0], 0 if ss is None else ss.shape[1],
                     x.data_ptr(), M_main, M, D, float(eps), rstd.data_ptr())
        return rstd

    def linear_residual_stats_(self, res: torch.Tensor, x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], eps: float):
        """res += x @ w^T (+ bias) in place, as linear_residual_, and the RMSNorm factor of every updated row: rstd [.] fp32.  The
        main rows' sums of squares come out of the dense layer's epilogue."""
        M, N = res.shape
        K = w.shape[1]
        Mm = self._nf_main_rows(M)
        ss = torch.empty(N // 128, (Mm + 255) // 256 * 256, dtype=torch.float32, device=res.device)
        self._main_then_sliver(M, M - Mm,
                               lambda Mm: self._launch("gemm_mfma", "evo_linear_mfma_nf_bf16", x.data_ptr(), w.data_ptr(), _ptr(bias), res.data_ptr(),
                                                       res.data_ptr(), None, ss.data_ptr(), ss.shape[1], Mm, N, K),
                               lambda Mm: self._linear_small_m(x[Mm:], w, bias, res[Mm:]))
        return self.rms_finalize(ss, res, Mm, eps)

    def linear_residual_yblk_stats_(self, res: torch.Tensor, y_blk: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], eps: float):
        """linear_residual_yblk_ + the RMSNorm factor of every updated row (see linear_residual_stats_)."""
        M, N = res.shape
        K = w.shape[1]
        r = self._sliver_rows(M, limit=255)
        ss = torch.empty(N // 128, M - r, dtype=torch.float32, device=res.device)
        self._main_then_sliver(M, r,
                               lambda Mf: self._launch("gemm_mfma", "evo_linear_xblk_mfma_nf_bf16", y_blk.data_ptr(), w.data_ptr(), _ptr(bias),
                                                       res.data_ptr(), res.data_ptr(), ss.data_ptr(), Mf, Mf, N, K),
                               lambda Mf: self.linear_residual_(res[Mf:], self._yblk_tail_rows(y_blk, Mf, M), w, bias=bias))
        return self.rms_finalize(ss, res, M - r, eps)

    def linear_rs(self, x: torch.Tensor, rstd: torch.Tensor, w_folded: torch.Tensor, b: Optional[torch.Tensor], w: torch.Tensor,
                  scale: torch.Tensor, eps: float) -> torch.Tensor:
        """linear(rmsnorm(x) * scale, w, b) with the norm as a row factor in the dense layer's epilogue: x is the raw stream, rstd its
        rows' factors, w_folded = fold_norm_scale(w, scale); the sliver rows take the norm-folding weight-streaming launch on w itself."""
        M, K = x.shape
        N = w.shape[0]
        Mm = self._nf_main_rows(M)
        y = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)

        def sliver(Mm):
            y[Mm:] = self.norm_linear(x[Mm:], scale, eps, w, b)
        self._main_then_sliver(M, M - Mm,
                               lambda Mm: self._launch("gemm_mfma", "evo_linear_mfma_nf_bf16", x.data_ptr(), w_folded.data_ptr(), _ptr(b), None,
                                                       y.data_ptr(), rstd.data_ptr(), None, 0, Mm, N, K),
                               sliver)
        return y

    def mlp_gate_rs(self, x: torch.Tensor, rstd: torch.Tensor, w12g_folded: torch.Tensor, w12: torch.Tensor, scale: torch.Tensor,
                    eps: float) -> torch.Tensor:
        """mlp_gate(rmsnorm(x) * scale, w12) with the norm as a row factor in the gated dense layer's epilogue (see linear_rs);
        w12g_folded = pack_gate_weights(fold_norm_scale(w12, scale))."""
        M, K = x.shape
        I = w12g_folded.shape[0] // 2
        Mm = self._nf_main_rows(M)
        a = torch.empty(M, I, dtype=torch.bfloat16, device=x.device)

        def sliver(Mm):
            a[Mm:] = self.mlp_gate(x[Mm:], w12, scale, eps, w12g=None if w12 is not None else w12g_folded)
        self._main_then_sliver(M, M - Mm,
                               lambda Mm: self._launch("gemm_gate", "evo_mlp_gate_mfma_nf_bf16", x.data_ptr(), rstd.data_ptr(), w12g_folded.data_ptr(),
                                                       a.data_ptr(), Mm, I, K),
                               sliver)
        return a

    def zt_stream_rows_ok(self, B: int, T: int) -> bool:
        """z^T layouts whose main area the swapped-operand projection can fill straight from the stream's rows (linear_t_rs): the tail
        form (rows of Tm = T - r positions: position b Tm + t = row b T + t), and the plain form when it has no pad position at all
        (T a multiple of 64 and B T a multiple of 256: position p = row p)."""
        Tm, Tp, Mp, r = self.zt_layout(B, T)
        if r > 0:
            return Tp == Tm and Mp == B * Tm and Tm % 256 == 0
        return Tp == T and Mp == B * T

    def linear_t_rs(self, x: torch.Tensor, rstd: torch.Tensor, w_folded: torch.Tensor, b: Optional[torch.Tensor], w: torch.Tensor,
                    scale: torch.Tensor, eps: float, B: int, T: int, tail: bool = True) -> torch.Tensor:
        """linear_t(rmsnorm_rows(x), w, b) without the normalised copy, for the layouts of zt_stream_rows_ok: the swapped-operand dense layer
        reads the raw stream x [B T, K] and scales by rstd in its epilogue; in the tail form the B r tail tokens take the norm-folding
        weight-streaming launch on w itself."""
        Tm, Tp, Mp, r = self.zt_layout(B, T)
        assert self.zt_stream_rows_ok(B, T)
        K = x.shape[1]
        N = w.shape[0]
        if r == 0:                                    # plain form without a single pad position: z^T position p IS row p of the stream
            zt = torch.empty(Mp // 256, N, 256, dtype=torch.bfloat16, device=x.device)
            self._launch("gemm_zt", "evo_linear_t_mfma_nf_bf16", x.data_ptr(), rstd.data_ptr(), w_folded.data_ptr(), _ptr(b), zt.data_ptr(),
                         Mp, N, K, Mp, Mp, 0)
            return zt
        zt = torch.empty(Mp // 256 + (1 if tail else 0), N, 256, dtype=torch.bfloat16, device=x.device)
        self._launch("gemm_zt", "evo_linear_t_mfma_nf_bf16", x.data_ptr(), rstd.data_ptr(), w_folded.data_ptr(), _ptr(b), zt.data_ptr(),
                     Mp, N, K, B * T, Tm, r)
        if tail:                                      # (else the caller runs the tail tokens through the single-token launch: hyena_ct(main_only=True))
            x_tail = x.view(B, T, K)[:, Tm:].reshape(B * r, K).contiguous()                       # (a copy of B r <= 16 rows)
            self._zt_tail_fill(zt, self.norm_linear(x_tail, scale, eps, w, b), B, r)
        return zt

    # The same operator in two stages, for sequence parallelism: stage 1 (launches 1+2) yields the shard's end
    # state from a ZERO carry-in; after the ranks exchange those, stage 2 (carry-add + launch 3) finishes.
    def hyena_stage1(self, z, fir_w, fir_b, poles, n_heads, z_halo=None, seg_len=None):
        self._need(z, torch.bfloat16, "hyena z")
        B, T, D3 = z.shape
        D = D3 // 3
        agg, C = self._hyena_seg_state(z, z_halo, fir_w, fir_b, poles, None, n_heads, seg_len)
        s_end = torch.empty(B, D, 8, 2, dtype=torch.float32, device=z.device)
        self._launch("hyena_carry_scan", "evo_hyena_carry_scan", agg.data_ptr(), poles.data_ptr(), None, s_end.data_ptr(), B, T, D, C)
        return (agg, C), torch.view_as_complex(s_end)

    def hyena_stage2(self, z, fir_w, fir_b, poles, residues, dskip, n_heads, stage1, z_halo=None, s0=None):
        agg, C = stage1
        B, T, D3 = z.shape
        D = D3 // 3
        if s0 is not None:
            s0r = torch.view_as_real(s0.to(torch.complex64).contiguous())
            self._launch("hyena_carry_add", "evo_hyena_carry_add", agg.data_ptr(), poles.data_ptr(), s0r.data_ptr(), B, T, D, C)
        return self._hyena_apply(z, z_halo, fir_w, fir_b, poles, residues, dskip, agg, None, n_heads, C)

    def hyena_step(self, z_t: torch.Tensor, fir_state: torch.Tensor, iir_state: torch.Tensor, fir_w, fir_b, poles,
                   residues, dskip, n_heads: int) -> torch.Tensor:
        """One decode step; fir_state [B,3D,2] bf16 and iir_state [B,D,8] complex64 are updated in place."""
        self._need(z_t, torch.bfloat16, "hyena_step z_t")
        self._need(fir_state, torch.bfloat16, "hyena_step fir_state")
        if iir_state.dtype != torch.complex64 or not iir_state.is_contiguous():
            raise RuntimeError("hyena_step: iir_state must be contiguous complex64")
        B, D3 = z_t.shape
        D = D3 // 3
        y = torch.empty(B, D, dtype=torch.bfloat16, device=z_t.device)
        sr = torch.view_as_real(iir_state)
        _check(self.lib.evo_hyena_step(z_t.data_ptr(), fir_state.data_ptr(), sr.data_ptr(), fir_w.data_ptr(),
                                       fir_b.data_ptr(), poles.data_ptr(), residues.data_ptr(), dskip.data_ptr(),
                                       y.data_ptr(), B, D, n_heads, _stream()), "evo_hyena_step")
        return y

    def hyena_decode_fused(self, x, norm_scale, eps, proj_w, proj_b, fir_state, iir_state, fir_w, fir_b, poles,
                           residues, dskip, n_heads: int) -> torch.Tensor:
        """One decode token through pre-norm + projections + FIR/modal step + gate in ONE launch (M = batch <= 4, or <= 8 at D = 4096);
        states are updated in place.  Falls back to the two kernels otherwise."""
        M, D = x.shape
        ok = (self.fused_rows_ok(M, D) and self._bf16_ok(x, proj_w, scale=norm_scale) and proj_b is not None
              and fir_state.dtype == torch.bfloat16 and fir_state.is_contiguous() and fir_state.shape[0] == M
              and iir_state.dtype == torch.complex64 and iir_state.is_contiguous() and iir_state.shape[0] == M
              and D == n_heads * 128)
        if not ok:
            z = self.norm_linear(x, norm_scale, eps, proj_w, proj_b)
            return self.hyena_step(z, fir_state, iir_state, fir_w, fir_b, poles, residues, dskip, n_heads)
        y = torch.empty(M, D, dtype=torch.bfloat16, device=x.device)
        sr = torch.view_as_real(iir_state)
        self._launch("gemv_hyena", "evo_hyena_decode_fused_small_m", x.data_ptr(), norm_scale.data_ptr(), proj_w.data_ptr(), proj_b.data_ptr(),
                     fir_state.data_ptr(), sr.data_ptr(), fir_w.data_ptr(), fir_b.data_ptr(), poles.data_ptr(), residues.data_ptr(),
                     dskip.data_ptr(), y.data_ptr(), M, D, n_heads, float(eps))
        return y

    def rope_(self, qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, q_scale: float = 1.0) -> torch.Tensor:
        """In-place NeoX rotary on the q and k thirds of qkv [B,T,3,H,hd].  `q_scale`: the rotated queries are multiplied by it before their
        one rounding (attn_q_scale(hd) when the attention that follows is called with prescaled=True; 1.0: plain rotary, exact)."""
        self._need(qkv, torch.bfloat16, "rope qkv")
        self._need(cos, torch.float32, "rope cos")
        self._need(sin, torch.float32, "rope sin")
        B, T, three, H, hd = qkv.shape
        assert three == 3 and cos.shape == (T, hd // 2)
        _check(self.lib.evo_rope_qk_bf16(qkv.data_ptr(), cos.data_ptr(), sin.data_ptr(), B, T, H, hd, float(q_scale), _stream()),
               "evo_rope_qk_bf16")
        return qkv

    def rope_append_decode(self, qkv: torch.Tensor, kv: torch.Tensor, pos: torch.Tensor, inv_freq: torch.Tensor,
                           scaling: float, q_scale: float = 1.0, widx: Optional[torch.Tensor] = None) -> None:
        """One decode token per stream: NeoX rotary on q and k of qkv [B,1,3,H,hd] (in place) at position pos[b] (/ scaling) and
        kv[b, pos[b]] = (k, v) -- kv [>=B, cap, 2, H, hd].  One launch; bit-identical to the rotary table + rope_ + indexed copy.
        `widx` (device int64 [B]): the row is written at kv[b, widx[b]] instead; the angle stays pos[b]'s (a cache that starts behind
        a prompt stored elsewhere: attention_decode_prefix)."""
        self._need(qkv, torch.bfloat16, "rope_append_decode qkv")
        B, T, three, H, hd = qkv.shape
        if T != 1 or three != 3 or kv.dtype != torch.bfloat16 or not kv.is_cuda or kv.stride(-1) != 1 or kv.shape[0] < B:
            raise RuntimeError("rope_append_decode: expects qkv [B,1,3,H,hd] and a bf16 KV cache [>=B,cap,2,H,hd]")
        self._check_address(kv.data_ptr(), "rope_append_decode kv")
        if pos.dtype != torch.int64 or not pos.is_cuda or pos.numel() != B or not pos.is_contiguous():
            raise RuntimeError("rope_append_decode pos: need a contiguous device int64 tensor with B entries")
        self._check_address(pos.data_ptr(), "rope_append_decode pos", 8)
        self._need(inv_freq, torch.float32, "rope_append_decode inv_freq")
        name, at = "evo_rope_append_decode_bf16", ()
        if widx is not None:
            if widx.dtype != torch.int64 or not widx.is_cuda or widx.numel() != B or not widx.is_contiguous():
                raise RuntimeError("rope_append_decode widx: need a contiguous device int64 tensor with B entries")
            self._check_address(widx.data_ptr(), "rope_append_decode widx", 8)
            name, at = "evo_rope_append_decode_at_bf16", (widx.data_ptr(),)
        _check(getattr(self.lib, name)(qkv.data_ptr(), kv.data_ptr(), pos.data_ptr(), inv_freq.data_ptr(), float(scaling), B, H, hd,
                                       kv.stride(0), kv.stride(1), kv.stride(2), kv.stride(3), float(q_scale), *at, _stream()), name)

    def attention(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, q_pos0: int, prescaled: bool = False) -> torch.Tensor:
        """Causal attention; q [B,Tq,H,128], k/v [B,Tk,H,128] (strided views allowed, last dim dense).  `prescaled`: q already carries
        softmax_scale * log2(e) (rope_'s q_scale = attn_q_scale(hd)): the 64-rows-per-wave kernel then runs without its per-score multiply."""
        self._need_strided("attention", q=q, k=k, v=v)
        B, Tq, H, hd = q.shape
        Tk = k.shape[1]
        if hd != 128:
            raise RuntimeError("attention: head dim must be 128")
        o = torch.empty(B, Tq, H, hd, dtype=torch.bfloat16, device=q.device)
        # query ranges longer than one 128-row block: the 64-rows-per-wave kernel, which reads V^T from a workspace its pre-pass fills
        vt = torch.empty(B, H, hd, (Tk + 63) // 64 * 64, dtype=torch.bfloat16, device=q.device) if (Tq > 128 and self.attn_w64) else None
        with self._t("attn_fwd"):
            _check(self.lib.evo_attn_fwd_causal_bf16(
                q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), B, H, Tq, Tk, int(q_pos0),
                q.stride(0), q.stride(1), q.stride(2), k.stride(0), k.stride(1), k.stride(2),
                v.stride(0), v.stride(1), v.stride(2), 0.0 if prescaled else 1.0 / math.sqrt(hd), _ptr(vt), _stream()), "evo_attn_fwd_causal_bf16")
        return o

    def attention_prefix_vt(self, v_pre: torch.Tensor, cols: Optional[int] = None) -> torch.Tensor:
        """The V^T plane [H, 128, cols] of a shared prefix v_pre [P, H, 128] (a strided view, e.g. kv[0, :P, 1] of a KV cache) for
        `attention_prefix`: built once per reference and layer, reused by every call whose prefix is the first P' <= P keys.  `cols`
        (default: P rounded up to 64) is the plane's row pitch."""
        if v_pre.dim() != 3 or v_pre.shape[2] != 128 or not v_pre.is_cuda or v_pre.dtype != torch.bfloat16 or v_pre.stride(-1) != 1:
            raise RuntimeError("attention_prefix_vt: need a ROCm bf16 tensor [P, H, 128] with a dense last dim")
        self._check_address(v_pre.data_ptr(), "attention_prefix_vt v_pre")
        P, H, hd = v_pre.shape
        cols = (P + 63) // 64 * 64 if cols is None else int(cols)
        if P < 1 or cols % 64 or cols < P:
            raise RuntimeError(f"attention_prefix_vt: {cols} columns for {P} keys (need a multiple of 64, >= P >= 1)")
        vt = torch.empty(H, hd, cols, dtype=torch.bfloat16, device=v_pre.device)
        with self._t("attn_prefix_vt"):
            _check(self.lib.evo_attn_prefix_vt_bf16(v_pre.data_ptr(), vt.data_ptr(), P, H, v_pre.stride(0), v_pre.stride(1), cols, _stream()),
                   "evo_attn_prefix_vt_bf16")
        return vt

    def attention_prefix(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, k_pre: torch.Tensor, v_pre: Optional[torch.Tensor],
                         vt_pre: Optional[torch.Tensor] = None, prescaled: bool = False) -> torch.Tensor:
        """Causal attention of B rows that share ONE prefix: q, k, v [B, Tq, H, 128] are the rows' own (suffix) tokens, k_pre / v_pre
        [P, H, 128] the prefix (no batch dimension; strided views allowed, e.g. kv[0, :P, 0] / kv[0, :P, 1] of a KV cache).  Query i of
        row b sees the P prefix keys and suffix keys 0 .. i of its row -- bit for bit `attention(q, cat(k_pre, k_b), cat(v_pre, v_b), P)`
        without the B copies.  vt_pre: the prefix's V^T plane from `attention_prefix_vt` (of these or MORE prefix keys), built here
        when None -- a caller with several groups per reference passes it.  P >= 64, P % 64 == 0 and Tq >= 129 (csrc/attn_w64.hip SEG)."""
        self._need_strided("attention_prefix", q=q, k=k, v=v, k_pre=k_pre, v_pre=v_pre, vt_pre=vt_pre)
        B, Tq, H, hd = q.shape
        if hd != 128 or k.shape != q.shape or v.shape != q.shape or k_pre.dim() != 3 or tuple(k_pre.shape[1:]) != (H, hd):
            raise RuntimeError("attention_prefix: expects q / k / v [B, Tq, H, 128] and k_pre [P, H, 128]")
        P = k_pre.shape[0]
        if P < 64 or P % 64 or Tq < 129:
            raise RuntimeError(f"attention_prefix: P = {P}, Tq = {Tq}: needs P >= 64, P % 64 == 0 and Tq >= 129")
        if vt_pre is None:
            if v_pre is None or tuple(v_pre.shape) != (P, H, hd):
                raise RuntimeError("attention_prefix: v_pre [P, H, 128] is needed to build the prefix's V^T plane")
            vt_pre = self.attention_prefix_vt(v_pre)
        if vt_pre.dim() != 3 or tuple(vt_pre.shape[:2]) != (H, hd) or not vt_pre.is_contiguous() or vt_pre.shape[2] % 64 or vt_pre.shape[2] < P:
            raise RuntimeError("attention_prefix vt_pre: need a contiguous [H, 128, cols] plane with cols % 64 == 0 and cols >= P")
        o = torch.empty(B, Tq, H, hd, dtype=torch.bfloat16, device=q.device)
        vt = torch.empty(B, H, hd, (Tq + 63) // 64 * 64, dtype=torch.bfloat16, device=q.device)
        with self._t("attn_prefix"):
            _check(self.lib.evo_attn_fwd_prefix_bf16(
                q.data_ptr(), k.data_ptr(), v.data_ptr(), k_pre.data_ptr(), vt_pre.data_ptr(), o.data_ptr(), B, H, Tq, P,
                q.stride(0), q.stride(1), q.stride(2), k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1), v.stride(2),
                k_pre.stride(0), k_pre.stride(1), vt_pre.shape[2], 0.0 if prescaled else 1.0 / math.sqrt(hd), vt.data_ptr(), _stream()),
                "evo_attn_fwd_prefix_bf16")
        return o

    def attention_decode(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                         pos: Optional[torch.Tensor] = None, n_splits: Optional[int] = None, prescaled: bool = False) -> torch.Tensor:
        """One query per sequence against the KV cache: q [B,1,H,128]; k/v [B,Tk,H,128] views.  With `pos`
        (device int64 [B], or [1] = same for every row) row b's query sits at pos[b] and sees keys [0,pos[b]];
        Tk is then just the capacity."""
        B, Tq, H, hd = q.shape
        if pos is not None:
            if pos.dtype != torch.int64 or not pos.is_cuda or pos.numel() not in (1, B):
                raise RuntimeError("attention_decode pos: need a device int64 tensor with 1 or B entries")
            pos = (pos.reshape(1).expand(B) if pos.numel() == 1 and B > 1 else pos.reshape(-1)).contiguous()
            self._check_address(pos.data_ptr(), "attention_decode pos", 8)
        if Tq != 1 or hd != 128:
            raise RuntimeError("attention_decode: expects [B,1,H,128] queries")
        self._need_strided("attention_decode", q=q, k=k, v=v)
        Tk = k.shape[1]
        n_splits = self._decode_splits(Tk) if n_splits is None else n_splits
        o = torch.empty(B, 1, H, hd, dtype=torch.bfloat16, device=q.device)
        part_o = torch.empty(B, H, n_splits, hd, dtype=torch.float32, device=q.device)
        part_ml = torch.empty(B, H, n_splits, 2, dtype=torch.float32, device=q.device)
        with self._t("attn_decode"):
            _check(self.lib.evo_attn_decode_bf16(
                q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), B, H, Tk, q.stride(0), q.stride(2),
                k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1), v.stride(2), _ptr(pos),
                part_o.data_ptr(), part_ml.data_ptr(), n_splits, 0.0 if prescaled else 1.0 / math.sqrt(hd), _stream()),
                "evo_attn_decode_bf16")
        return o

    attn_group_rows = ATTN_GROUP_ROWS

    @staticmethod
    def _decode_splits(n_keys: int) -> int:
        """Splits of a decode attention over n_keys keys: one per WAVE of the streaming kernel, whole workgroups of four, at most one per
        64-key block, at most 32.  Measured on MI355X (tools/experiments/attn_decode_bench.py, round 6: the kernel keeps the next 32-key
        half's requests in flight while it reduces the current one): 32 is best from 8 k to 131 k keys at batch 1-3 (29.5 / 78.7 / 102 /
        384 us at 1 x 8 k / 3 x 8 k / 32 k / 131 k; 64 splits: 31.7 / 81.3 / 107 / 385; the load-then-reduce loop of rounds 3-5 wanted 64
        and took 36.8 / 94.5 / 118 / 428)."""
        return min(((n_keys + 63) // 64 + 3) // 4 * 4, 32)

    def attention_decode_prefix(self, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, own_pos: torch.Tensor,
                                k_store: torch.Tensor, v_store: torch.Tensor, pre_row: torch.Tensor, pre_len: torch.Tensor,
                                n_splits: Optional[int] = None, n_pre_splits: Optional[int] = None, prescaled: bool = False) -> torch.Tensor:
        """One query per row behind a SHARED prompt: q [B,1,H,128]; k / v [B,cap,H,128] the rows' own caches, row b holds keys
        [0, own_pos[b]]; k_store / v_store [R,P_cap,H,128] views of a prompt store, pre_row [B] the store row each batch row continues
        (-1: none), pre_len [R] the keys each store row holds.  Row b sees the store row's keys, then its own -- `attention_decode` on the
        concatenation without a copy of the prompt per row.  All four index vectors are device int64 (nothing is read back)."""
        B, Tq, H, hd = q.shape
        if Tq != 1 or hd != 128:
            raise RuntimeError("attention_decode_prefix: expects [B,1,H,128] queries")
        self._need_strided("attention_decode_prefix", 4, q=q, k=k, v=v, k_store=k_store, v_store=v_store)
        R, P_cap = k_store.shape[:2]
        if k.shape[0] < B or v.shape != k.shape or tuple(k.shape[2:]) != (H, hd) or v_store.shape != k_store.shape or tuple(k_store.shape[2:]) != (H, hd) \
                or R < 1 or P_cap < 1:
            raise RuntimeError("attention_decode_prefix: expects k / v [B,cap,H,128] and k_store / v_store [R,P_cap,H,128]")
        for t, n, nm in ((own_pos, B, "own_pos"), (pre_row, B, "pre_row"), (pre_len, R, "pre_len")):
            if t.dtype != torch.int64 or not t.is_cuda or t.numel() != n or not t.is_contiguous():
                raise RuntimeError(f"attention_decode_prefix {nm}: need a contiguous device int64 tensor with {n} entries")
            self._check_address(t.data_ptr(), f"attention_decode_prefix {nm}", 8)
        Tk = k.shape[1]
        n_splits = self._decode_splits(Tk) if n_splits is None else int(n_splits)
        n_pre_splits = self._decode_splits(P_cap) if n_pre_splits is None else int(n_pre_splits)
        n_tot = n_splits + n_pre_splits
        o = torch.empty(B, 1, H, hd, dtype=torch.bfloat16, device=q.device)
        part_o = torch.empty(B, H, n_tot, hd, dtype=torch.float32, device=q.device)
        part_ml = torch.empty(B, H, n_tot, 2, dtype=torch.float32, device=q.device)
        with self._t("attn_decode_prefix"):
            _check(self.lib.evo_attn_decode_prefix_bf16(
                q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), B, H, Tk, q.stride(0), q.stride(2),
                k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1), v.stride(2), own_pos.data_ptr(),
                k_store.data_ptr(), v_store.data_ptr(), R, P_cap, k_store.stride(0), k_store.stride(1), k_store.stride(2),
                v_store.stride(0), v_store.stride(1), v_store.stride(2), pre_row.data_ptr(), pre_len.data_ptr(),
                part_o.data_ptr(), part_ml.data_ptr(), n_pre_splits, n_splits, 0.0 if prescaled else 1.0 / math.sqrt(hd), _stream()),
                "evo_attn_decode_prefix_bf16")
        return o

    # ---- FP8 (e4m3fn) KV cache: the optional group "kv_fp8" (csrc/kv_fp8.hip) --------------------------------------
    def _fp8_cache_args(self, op: str, kv, B: int, H: int) -> tuple:
        """The cache operand of the three FP8 launches, checked: kv.data [>=B, cap, 2, H, 128] uint8, kv.scale [>=B, 2, H, cap] f32 with
        contiguous tokens -> (data ptr, scale ptr, the seven strides)."""
        d, s = kv.data, kv.scale
        if not d.is_cuda or not s.is_cuda or d.dtype != torch.uint8 or s.dtype != torch.float32 or d.dim() != 5 or s.dim() != 4:
            raise RuntimeError(f"{op}: the FP8 cache is data [B,cap,2,H,128] uint8 + scale [B,2,H,cap] f32 on a ROCm device")
        cap = d.shape[1]
        if d.shape[0] < B or tuple(d.shape[2:]) != (2, H, 128) or d.stride(-1) != 1 or s.shape[0] < B or tuple(s.shape[1:]) != (2, H, cap) \
                or s.stride(-1) != 1:
            raise RuntimeError(f"{op}: cache shapes {tuple(d.shape)} / {tuple(s.shape)} do not fit B = {B}, H = {H}, head dim 128")
        self._check_address(d.data_ptr(), f"{op} kv.data")
        self._check_address(s.data_ptr(), f"{op} kv.scale", 4)
        return (d.data_ptr(), s.data_ptr(), d.stride(0), d.stride(1), d.stride(2), d.stride(3), s.stride(0), s.stride(1), s.stride(2))

    def kv_quant_fp8(self, k: torch.Tensor, v: torch.Tensor, kv, t0: int = 0) -> None:
        """Rows k, v [B, T, H, 128] bf16 (strided views: the thirds of a packed qkv) -> tokens t0 .. t0 + T - 1 of the FP8 cache `kv`
        (an Fp8KV: data [>=B, cap, 2, H, 128] uint8, scale [>=B, 2, H, cap] f32), by the rule of include/evo_mi355x.h."""
        self._need_strided("kv_quant_fp8", 4, k=k, v=v)
        B, T, H, hd = k.shape
        if hd != 128 or v.shape != k.shape:
            raise RuntimeError("kv_quant_fp8: expects k / v [B, T, H, 128]")
        ptrs = self._fp8_cache_args("kv_quant_fp8", kv, B, H)
        cap = kv.data.shape[1]
        if t0 < 0 or t0 + T > cap:
            raise RuntimeError(f"kv_quant_fp8: tokens [{t0}, {t0 + T}) do not fit a cache of {cap}")
        with self._t("kv_quant_fp8"):
            _check(self.lib.evo_kv_quant_fp8(k.data_ptr(), v.data_ptr(), ptrs[0], ptrs[1], B, T, H, int(t0), cap,
                                             k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1), v.stride(2), *ptrs[2:],
                                             _stream()), "evo_kv_quant_fp8")

    def rope_append_decode_fp8(self, qkv: torch.Tensor, kv, pos: torch.Tensor, inv_freq: torch.Tensor, scaling: float,
                               q_scale: float = 1.0) -> None:
        """`rope_append_decode` on an FP8 cache: the same rotary on q and k of qkv [B,1,3,H,128] (bit for bit), then k and v quantised
        into token pos[b] of `kv` (an Fp8KV).  One launch."""
        self._need(qkv, torch.bfloat16, "rope_append_decode_fp8 qkv")
        B, T, three, H, hd = qkv.shape
        if T != 1 or three != 3 or hd != 128:
            raise RuntimeError("rope_append_decode_fp8: expects qkv [B,1,3,H,128]")
        ptrs = self._fp8_cache_args("rope_append_decode_fp8", kv, B, H)
        if pos.dtype != torch.int64 or not pos.is_cuda or pos.numel() != B or not pos.is_contiguous():
            raise RuntimeError("rope_append_decode_fp8 pos: need a contiguous device int64 tensor with B entries")
        self._check_address(pos.data_ptr(), "rope_append_decode_fp8 pos", 8)
        self._need(inv_freq, torch.float32, "rope_append_decode_fp8 inv_freq")
        _check(self.lib.evo_rope_append_decode_fp8(qkv.data_ptr(), ptrs[0], ptrs[1], pos.data_ptr(), inv_freq.data_ptr(), float(scaling),
                                                   B, H, hd, *ptrs[2:], float(q_scale), _stream()), "evo_rope_append_decode_fp8")

    def attention_decode_fp8(self, q: torch.Tensor, kv, pos: Optional[torch.Tensor] = None, n_keys: Optional[int] = None,
                             n_splits: Optional[int] = None, prescaled: bool = False) -> torch.Tensor:
        """`attention_decode` on an FP8 cache: q [B,1,H,128] against `kv` (an Fp8KV).  With `pos` (device int64 [B] or [1]) row b sees
        keys [0, pos[b]] and the cache's capacity is only the bound; without it every row sees the first `n_keys` keys."""
        B, Tq, H, hd = q.shape
        if pos is not None:
            if pos.dtype != torch.int64 or not pos.is_cuda or pos.numel() not in (1, B):
                raise RuntimeError("attention_decode_fp8 pos: need a device int64 tensor with 1 or B entries")
            pos = (pos.reshape(1).expand(B) if pos.numel() == 1 and B > 1 else pos.reshape(-1)).contiguous()
            self._check_address(pos.data_ptr(), "attention_decode_fp8 pos", 8)
        if Tq != 1 or hd != 128:
            raise RuntimeError("attention_decode_fp8: expects [B,1,H,128] queries")
        self._need_strided("attention_decode_fp8", q=q)
        ptrs = self._fp8_cache_args("attention_decode_fp8", kv, B, H)
        cap = kv.data.shape[1]
        Tk = cap if pos is not None or n_keys is None else int(n_keys)
        if Tk < 1 or Tk > cap:
            raise RuntimeError(f"attention_decode_fp8: {Tk} keys in a cache of {cap}")
        n_splits = self._decode_splits(Tk) if n_splits is None else n_splits
        o = torch.empty(B, 1, H, hd, dtype=torch.bfloat16, device=q.device)
        part_o = torch.empty(B, H, n_splits, hd, dtype=torch.float32, device=q.device)
        part_ml = torch.empty(B, H, n_splits, 2, dtype=torch.float32, device=q.device)
        with self._t("attn_decode_fp8"):
            _check(self.lib.evo_attn_decode_fp8(q.data_ptr(), ptrs[0], ptrs[1], o.data_ptr(), B, H, Tk, q.stride(0), q.stride(2), *ptrs[2:],
                                                _ptr(pos), part_o.data_ptr(), part_ml.data_ptr(), n_splits,
                                                0.0 if prescaled else 1.0 / math.sqrt(hd), _stream()), "evo_attn_decode_fp8")
        return o

    # ---- paged bf16 KV cache: the optional group "kv_paged" (csrc/kv_paged.hip) ----------------------------------------
    def _paged_cache_args(self, op: str, kv, B: int, H: int) -> tuple:
        """The cache operand of the two paged launches, checked: kv.pages [n_pages, page_tokens, 2, H, 128] bf16, kv.table [>=B, width]
        int32 with contiguous rows -> (pages ptr, table ptr, page_tokens, n_pages, table_width, the four strides).  The table is not read."""
        p, t = kv.pages, kv.table
        if not p.is_cuda or not t.is_cuda or p.dtype != torch.bfloat16 or t.dtype != torch.int32 or p.dim() != 5 or t.dim() != 2:
            raise RuntimeError(f"{op}: the paged cache is pages [n_pages,page_tokens,2,H,128] bf16 + table [B,width] int32 on a ROCm device")
        pt = p.shape[1]
        if tuple(p.shape[2:]) != (2, H, 128) or p.stride(-1) != 1 or p.shape[0] < 1 or pt < 64 or pt & (pt - 1) or t.shape[0] < B \
                or t.shape[1] < 1 or t.stride(1) != 1 or (t.shape[0] > 1 and t.stride(0) != t.shape[1]):
            raise RuntimeError(f"{op}: cache shapes {tuple(p.shape)} / {tuple(t.shape)} do not fit B = {B}, H = {H}, head dim 128, "
                               "page_tokens a power of two >= 64")
        self._check_address(p.data_ptr(), f"{op} kv.pages")
        self._check_address(t.data_ptr(), f"{op} kv.table", 4)
        return (p.data_ptr(), t.data_ptr(), pt, p.shape[0], t.shape[1], p.stride(0), p.stride(1), p.stride(2), p.stride(3))

    def rope_append_decode_paged(self, qkv: torch.Tensor, kv, pos: torch.Tensor, inv_freq: torch.Tensor, scaling: float,
                                 q_scale: float = 1.0) -> None:
        """`rope_append_decode` on a paged cache: the same rotary on q and k of qkv [B,1,3,H,128] (bit for bit), then k and v go to token
        pos[b] of row b's pages (`kv`: a PagedKV).  One launch."""
        self._need(qkv, torch.bfloat16, "rope_append_decode_paged qkv")
        B, T, three, H, hd = qkv.shape
        if T != 1 or three != 3 or hd != 128:
            raise RuntimeError("rope_append_decode_paged: expects qkv [B,1,3,H,128]")
        a = self._paged_cache_args("rope_append_decode_paged", kv, B, H)
        if pos.dtype != torch.int64 or not pos.is_cuda or pos.numel() != B or not pos.is_contiguous():
            raise RuntimeError("rope_append_decode_paged pos: need a contiguous device int64 tensor with B entries")
        self._check_address(pos.data_ptr(), "rope_append_decode_paged pos", 8)
        self._need(inv_freq, torch.float32, "rope_append_decode_paged inv_freq")
        _check(self.lib.evo_rope_append_decode_paged_bf16(qkv.data_ptr(), a[0], a[1], pos.data_ptr(), inv_freq.data_ptr(), float(scaling),
                                                          B, H, hd, *a[2:], float(q_scale), _stream()), "evo_rope_append_decode_paged_bf16")

    def attention_decode_paged(self, q: torch.Tensor, kv, pos: torch.Tensor, n_splits: Optional[int] = None,
                               prescaled: bool = False) -> torch.Tensor:
        """`attention_decode` on a paged cache: q [B,1,H,128] against `kv` (a PagedKV); row b sees keys [0, pos[b]] of its pages (pos:
        device int64 [B], required).  A row is bounded by table_width * page_tokens keys, which also sets the default `n_splits`."""
        B, Tq, H, hd = q.shape
        if pos is None or pos.dtype != torch.int64 or not pos.is_cuda or pos.numel() != B:
            raise RuntimeError("attention_decode_paged pos: need a device int64 tensor with B entries")
        pos = pos.reshape(-1).contiguous()
        self._check_address(pos.data_ptr(), "attention_decode_paged pos", 8)
        if Tq != 1 or hd != 128:
            raise RuntimeError("attention_decode_paged: expects [B,1,H,128] queries")
        self._need_strided("attention_decode_paged", q=q)
        a = self._paged_cache_args("attention_decode_paged", kv, B, H)
        n_splits = self._decode_splits(a[4] * a[2]) if n_splits is None else int(n_splits)
        o = torch.empty(B, 1, H, hd, dtype=torch.bfloat16, device=q.device)
        part_o = torch.empty(B, H, n_splits, hd, dtype=torch.float32, device=q.device)
        part_ml = torch.empty(B, H, n_splits, 2, dtype=torch.float32, device=q.device)
        with self._t("attn_decode_paged"):
            _check(self.lib.evo_attn_decode_paged_bf16(q.data_ptr(), a[0], a[1], o.data_ptr(), B, H, a[2], a[3], a[4], q.stride(0), q.stride(2),
                                                       *a[5:], pos.data_ptr(), part_o.data_ptr(), part_ml.data_ptr(), n_splits,
                                                       0.0 if prescaled else 1.0 / math.sqrt(hd), _stream()), "evo_attn_decode_paged_bf16")
        return o

    # ---- row-invariant dense launches: the optional group "row_invariant" (csrc/gemv_inv.hip) ----
    # One form per layer shape for 1-64 rows: row i of an M-row call is bit for bit the one-row call on row i.  A shape outside the contract
    # (K % 256, N % 64, I % 32) is an error: another form would sum in another order.
    def _linear_rowinv(self, x, w, b, res):
        M, K = x.shape
        N = w.shape[0]
        if not self._bf16_ok(x, w) or (b is not None and not self._bf16_ok(b)) or (res is not None and not self._bf16_ok(res)):
            raise RuntimeError("linear_rowinv: operands must be contiguous ROCm bf16 tensors")
        if not 1 <= M <= 64 or K % 256 or N % 64 or w.shape[1] != K:
            raise RuntimeError(f"linear_rowinv: x {tuple(x.shape)} against w {tuple(w.shape)}: need 1-64 rows, K % 256 == 0, N % 64 == 0")
        y = res if res is not None else torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
        ws = torch.empty(8 * M * N, dtype=torch.float32, device=x.device) if N < 8192 else None     # the K slices' partial sums
        self._launch("gemv_rowinv", "evo_linear_rowinv_bf16", x.data_ptr(), w.data_ptr(), _ptr(b), _ptr(res), y.data_ptr(), M, N, K, _ptr(ws),
                     0 if ws is None else ws.numel() * 4)
        return y

    def linear_rowinv(self, x: torch.Tensor, w: torch.Tensor, b: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x [M, K] @ w [N, K]^T (+ b) -> [M, N] bf16, every row computed as if it were alone (1 <= M <= 64)."""
        return self._linear_rowinv(x, w, b, None)

    def linear_residual_rowinv_(self, res: torch.Tensor, x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        """res += x @ w^T (+ bias) in place (fp32 accumulate, one rounding), every row computed as if it were alone."""
        return self._linear_rowinv(x, w, bias, res)

    def mlp_gate_rowinv(self, x: torch.Tensor, w12: Optional[torch.Tensor], w12g: Optional[torch.Tensor] = None) -> torch.Tensor:
        """a [M, I] = gelu(x @ W1^T) * (x @ W2^T) on rows x that are already normalised; w12 = [W1; W2], or (w12 None) the regrouped w12g."""
        M, K = x.shape
        wsrc = w12 if w12 is not None else w12g
        I = wsrc.shape[0] // 2
        if not self._bf16_ok(x, wsrc):
            raise RuntimeError("mlp_gate_rowinv: operands must be contiguous ROCm bf16 tensors")
        if not 1 <= M <= 64 or K % 256 or I % 32 or wsrc.shape[1] != K:
            raise RuntimeError(f"mlp_gate_rowinv: x {tuple(x.shape)} against w12 {tuple(wsrc.shape)}: need 1-64 rows, K % 256 == 0, I % 32 == 0")
        a = torch.empty(M, I, dtype=torch.bfloat16, device=x.device)
        self._launch("gemv_gate_rowinv", "evo_mlp_gate_rowinv_bf16", x.data_ptr(), wsrc.data_ptr(), a.data_ptr(), M, I, K, 1 if w12 is None else 0)
        return a

    # ---- FP8 (e4m3fn) weights for the single-token step: the optional group "w_fp8" (1-8 rows: csrc/gemv_fp8.hip, DESIGN.md section 22;
    # 9-64 rows: csrc/skinny_fp8.hip, the MFMA weight-streaming forms) ----
    # Each method is its bf16 namesake with an Fp8Weight record in place of the weight, and takes the same route: fused where the bf16
    # launch is fused (Backend.fused_rows_ok), norm pass + plain launch where it is not.  Nothing here falls back to bf16 weights.
    def _w8_args(self, op: str, x: torch.Tensor, rec) -> tuple:
        """(data ptr, scale ptr) of `rec` checked against x [M, K]: uint8 [N, K] + f32 [N] on x's device, K % 16 == 0, 1 <= M <= 64 (from
        9 rows on K % 256 == 0: the MFMA forms of csrc/skinny_fp8.hip)."""
        self._need(x, torch.bfloat16, f"{op} x")
        d, sc = rec.data, rec.scale
        M, K = x.shape
        if not d.is_cuda or not sc.is_cuda or d.dtype != torch.uint8 or sc.dtype != torch.float32 or d.dim() != 2 or not d.is_contiguous() \
                or not sc.is_contiguous() or tuple(sc.shape) != (d.shape[0],):
            raise RuntimeError(f"{op}: an FP8 weight is data [N, K] uint8 + scale [N] f32, contiguous, on a ROCm device")
        if d.shape[1] != K or K % 16 or not 1 <= M <= self.W8_ROWS:
            raise RuntimeError(f"{op}: x {tuple(x.shape)} against an FP8 weight {tuple(d.shape)}: need matching K % 16 == 0 and 1-{self.W8_ROWS} rows")
        if M > 8 and K % 256:
            raise RuntimeError(f"{op}: x {tuple(x.shape)} against an FP8 weight {tuple(d.shape)}: 9-{self.W8_ROWS} rows need K % 256 == 0")
        self._check_address(d.data_ptr(), f"{op} weight data")
        self._check_address(sc.data_ptr(), f"{op} weight scale", 4)
        return d.data_ptr(), sc.data_ptr()

    def w_quant_fp8(self, w: torch.Tensor):
        """w [N, K] bf16 -> Fp8Weight(data [N, K] uint8, scale [N] f32) by the rule of include/evo_mi355x.h (ABI 20).  One launch."""
        from .sh.cache import Fp8Weight
        self._need(w, torch.bfloat16, "w_quant_fp8 w")
        N, K = w.shape
        if K % 16:
            raise RuntimeError(f"w_quant_fp8: K = {K} is not a multiple of 16")
        rec = Fp8Weight(torch.empty(N, K, dtype=torch.uint8, device=w.device), torch.empty(N, dtype=torch.float32, device=w.device))
        self._launch("w_quant_fp8", "evo_w_quant_fp8", w.data_ptr(), rec.data.data_ptr(), rec.scale.data_ptr(), N, K)
        return rec

    def _linear_w8(self, x, rec, b, res):
        wd, ws = self._w8_args("linear_w8", x, rec)
        M, K = x.shape
        N = rec.data.shape[0]
        if res is not None:
            self._need(res, torch.bfloat16, "linear_w8 residual")
        y = res if res is not None else torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
        if M > 8:                                                # 9-64 rows: the MFMA weight-streaming forms (csrc/skinny_fp8.hip)
            part = self._skinny_w8_ws(x.device, M, N, K)
            self._launch("skinny_w8", "evo_linear_skinny_w8", x.data_ptr(), wd, ws, _ptr(b), _ptr(res), y.data_ptr(), M, N, K, _ptr(part),
                         0 if part is None else part.numel() * 4)
            return y
        self._launch("gemv_w8", "evo_linear_small_m_w8", x.data_ptr(), wd, ws, _ptr(b), _ptr(res), y.data_ptr(), M, N, K, None, 0)
        return y

    def _skinny_w8_ws(self, device, M: int, N: int, K: int) -> Optional[torch.Tensor]:
        """The workspace of evo_linear_skinny_w8's split over K (narrow layers: N < 8192, N % 64 == 0, two 256-k units or more), one per
        (thread, device, M, N) until release_workspaces(): a decode step calls this twice per block, and inside a graph capture every
        fresh tensor is memory the graph's pool keeps.  A thread's launches on its stream run in order, so they share it.  (A captured
        graph holds the address: release_workspaces() is for code that owns no live graph, as with the rmsnorm_rows workspace.)"""
        if N >= 8192 or N % 64 or K < 512:
            return None
        cache = getattr(self._xpad, "w8_ws", None)
        if cache is None:
            cache = self._xpad.w8_ws = {}
        key = (device.index, M, N)
        part = cache.get(key)
        if part is None:
            part = cache[key] = torch.empty(8 * M * N, dtype=torch.float32, device=device)
        return part

    def linear_w8(self, x: torch.Tensor, rec, b: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x [M, K] @ W^T (+ b) -> [M, N] bf16, W an Fp8Weight, 1 <= M <= 64 (K % 256 == 0 from 9 rows on)."""
        return self._linear_w8(x, rec, b, None)

    def linear_residual_w8_(self, res: torch.Tensor, x: torch.Tensor, rec, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
        """res += x @ W^T (+ bias), in place, one rounding."""
        return self._linear_w8(x, rec, bias, res)

    def norm_linear_w8(self, x: torch.Tensor, scale: torch.Tensor, eps: float, rec, b: Optional[torch.Tensor] = None) -> torch.Tensor:
        """linear_w8(rmsnorm(x) * scale, W, b): one launch where norm_linear has one."""
        M, K = x.shape
        N = rec.data.shape[0]
        if self.fused_rows_ok(M, K) and N > 4096 and self._bf16_ok(x, scale=scale):
            wd, ws = self._w8_args("norm_linear_w8", x, rec)
            y = torch.empty(M, N, dtype=torch.bfloat16, device=x.device)
            self._launch("gemv_norm_w8", "evo_norm_linear_small_m_w8", x.data_ptr(), scale.data_ptr(), wd, ws, _ptr(b), y.data_ptr(), M, N, K,
                         float(eps))
            return y
        return self.linear_w8(self.rmsnorm(x, None, scale, eps), rec, b)

    def hyena_decode_fused_w8(self, x, norm_scale, eps, rec, proj_b, fir_state, iir_state, fir_w, fir_b, poles, residues, dskip,
                              n_heads: int) -> torch.Tensor:
        """hyena_decode_fused on an FP8 projection weight: one launch at the rows where that has one, norm_linear_w8 + hyena_step otherwise."""
        M, D = x.shape
        ok = (self.fused_rows_ok(M, D) and self._bf16_ok(x, scale=norm_scale) and proj_b is not None
              and fir_state.dtype == torch.bfloat16 and fir_state.is_contiguous() and fir_state.shape[0] == M
              and iir_state.dtype == torch.complex64 and iir_state.is_contiguous() and iir_state.shape[0] == M
              and D == n_heads * 128)
        if not ok:
            z = self.norm_linear_w8(x, norm_scale, eps, rec, proj_b)
            return self.hyena_step(z, fir_state, iir_state, fir_w, fir_b, poles, residues, dskip, n_heads)
        wd, ws = self._w8_args("hyena_decode_fused_w8", x, rec)
        if rec.data.shape[0] != 3 * D:
            raise RuntimeError(f"hyena_decode_fused_w8: the projection weight must be [3 D, D], got {tuple(rec.data.shape)}")
        y = torch.empty(M, D, dtype=torch.bfloat16, device=x.device)
        sr = torch.view_as_real(iir_state)
        self._launch("gemv_hyena_w8", "evo_hyena_decode_fused_small_m_w8", x.data_ptr(), norm_scale.data_ptr(), wd, ws, proj_b.data_ptr(),
                     fir_state.data_ptr(), sr.data_ptr(), fir_w.data_ptr(), fir_b.data_ptr(), poles.data_ptr(), residues.data_ptr(),
                     dskip.data_ptr(), y.data_ptr(), M, D, n_heads, float(eps))
        return y

    def mlp_gate_w8(self, x: torch.Tensor, rec, norm_scale: Optional[torch.Tensor] = None, eps: float = 0.0, grouped: bool = False) -> torch.Tensor:
        """a [M, I] = gelu(x' @ W1^T) * (x' @ W2^T) with [W1; W2] an Fp8Weight ([2 I, K]; `grouped`: in pack_gate_weights' row order);
        x' = x, or rmsnorm(x) * norm_scale.  One launch where the rows allow the fold, norm pass + one launch otherwise."""
        M, K = x.shape
        I = rec.data.shape[0] // 2
        if norm_scale is not None and not (self.fused_rows_ok(M, K) and self._bf16_ok(x, scale=norm_scale)):
            x, norm_scale = self.rmsnorm(x, None, norm_scale, eps), None
        wd, ws = self._w8_args("mlp_gate_w8", x, rec)
        if I % 2 or (grouped and I % 32):
            raise RuntimeError(f"mlp_gate_w8: inner size {I} does not fit the launch (even; a multiple of 32 in the grouped order)")
        a = torch.empty(M, I, dtype=torch.bfloat16, device=x.device)
        if M > 8:                                                # (norm_scale is None here: fused_rows_ok ends at 8 rows)
            if I % 32:
                raise RuntimeError(f"mlp_gate_w8: inner size {I} is not a multiple of 32 (the 9-{self.W8_ROWS}-row launch)")
            self._launch("skinny_gate_w8", "evo_mlp_gate_skinny_w8", x.data_ptr(), wd, ws, a.data_ptr(), M, I, K, int(bool(grouped)))
            return a
        if norm_scale is None:
            self._launch("gemv_gate_w8", "evo_mlp_gate_small_m_w8", x.data_ptr(), wd, ws, a.data_ptr(), M, I, K, int(bool(grouped)))
        else:
            self._launch("gemv_gate_w8", "evo_norm_mlp_gate_small_m_w8", x.data_ptr(), norm_scale.data_ptr(), wd, ws, a.data_ptr(), M, I, K,
                         float(eps), int(bool(grouped)))
        return a

    def norm_linear(self, x: torch.Tensor, scale: torch.Tensor, eps: float, w: torch.Tensor,
                    b: Optional[torch.Tensor] = None, mfma: bool = False) -> torch.Tensor:
        """linear(rmsnorm(x) * scale, w, b).  Decode-sized batches (M <= 4) with a wide layer take ONE weight-streaming
        launch that rebuilds the normalised row on the fly; everything else is the two kernels."""
        M, K = x.shape
        if self.fused_rows_ok(M, K) and w.shape[0] > 4096 and self._bf16_ok(x, w, scale=scale) and K % 8 == 0:
            y = torch.empty(M, w.shape[0], dtype=torch.bfloat16, device=x.device)
            self._launch("gemv_norm", "evo_norm_linear_small_m_bf16", x.data_ptr(), scale.data_ptr(), w.data_ptr(), _ptr(b), y.data_ptr(),
                         M, w.shape[0], K, float(eps))
            return y
        return self.linear(self.rmsnorm(x, None, scale, eps), w, b, mfma=mfma)

    def mlp_gate_fused_ok(self, x: torch.Tensor, w12g: Optional[torch.Tensor]) -> bool:
        """The one-launch form of the gated MLP's first half (csrc/gemm.hip, gated epilogue) takes prefill-sized batches."""
        if w12g is None or not self.mlp_gate_fused:
            return False
        M, K = x.shape
        return M >= 256 and self._gemm_shape_ok(M, w12g.shape[0], K) and self._bf16_ok(x, w12g)

    def mlp_gate(self, x: torch.Tensor, w12: Optional[torch.Tensor], norm_scale: Optional[torch.Tensor] = None,
                 eps: float = 0.0, w12g: Optional[torch.Tensor] = None) -> torch.Tensor:
        """a [M, I] = gelu(x' @ W1^T) * (x' @ W2^T), w12 = [W1; W2] ([2I, K]); x' = x, or rmsnorm(x) * norm_scale when
        `norm_scale` is given.  Decode-sized batches (M <= 4) take ONE weight-streaming launch; prefill-sized ones the
        matrix-core dense layer with the gate in its epilogue when `w12g` (pack_gate_weights(w12)) is given -- the
        [M, 2 I] intermediate is never written; everything else is (norm,) dense layer and gate kernel.
        `w12 = None` (round 6, one weight set: StripedHyena.fold_norms_): only the regrouped copy w12g exists -- the weight-streaming
        launches read it in that row order (`grouped`), the unfused fallback un-groups the dense layer's columns."""
        M, K = x.shape
        wsrc = w12 if w12 is not None else w12g
        grouped = 1 if w12 is None else 0
        I = wsrc.shape[0] // 2
        if self.mlp_gate_fused_ok(x, w12g):
            if norm_scale is not None:
                x = self.rmsnorm(x, None, norm_scale, eps)
            a = torch.empty(M, I, dtype=torch.bfloat16, device=x.device)

            def sliver(Mm):                                       # the BOS sliver (M % 256 <= 16) goes through the small-M path
                a[Mm:] = self.mlp_gate(x[Mm:], w12, w12g=w12g if w12 is None else None)
            self._main_then_sliver(M, self._tail_rows(x, wsrc),
                                   lambda Mm: self._launch("gemm_gate", "evo_mlp_gate_mfma_bf16", x.data_ptr(), w12g.data_ptr(), a.data_ptr(), Mm, I, K),
                                   sliver)
            return a
        ok_mem = self._bf16_ok(x, wsrc, scale=norm_scale)
        # (5-8 rows WITH a norm keep the dot2 launch that norms for itself: one launch -- the BOS sliver of a scoring batch -- against norm pass + 44 us)
        if self.gate_small_m_mfma and 5 <= M <= 64 and (M > 8 or norm_scale is None) and K % 256 == 0 and I % 32 == 0 and ok_mem:
            # round 6: 5-64 rows on the MFMA weight-streaming form with the gate in its epilogue (csrc/gemv.hip skinny_nw_kernel GATE; 512-byte weight
            # requests, x shared by the workgroup: 5.4 TB/s of weights at 8 rows where the dot2 launch runs 3.6); the norm as its own small pass in front
            if norm_scale is not None:
                x = self.rmsnorm(x, None, norm_scale, eps)
            a = torch.empty(M, I, dtype=torch.bfloat16, device=x.device)
            self._launch("gemv_gate", "evo_mlp_gate_small_m_bf16", x.data_ptr(), wsrc.data_ptr(), a.data_ptr(), M, I, K, grouped)
            return a
        # (without a norm the dot2 launch stops at 4 rows: 5-8 rows are the MFMA form's above, or the dense layer's)
        if ((1 <= M <= 4 or norm_scale is not None) and self.fused_rows_ok(M, K) and ok_mem and K % 8 == 0 and I % 2 == 0
                and (not grouped or I % 32 == 0)):
            a = torch.empty(M, I, dtype=torch.bfloat16, device=x.device)
            if norm_scale is None:
                self._launch("gemv_gate", "evo_mlp_gate_small_m_bf16", x.data_ptr(), wsrc.data_ptr(), a.data_ptr(), M, I, K, grouped)
            else:
                self._launch("gemv_gate", "evo_norm_mlp_gate_small_m_bf16", x.data_ptr(), norm_scale.data_ptr(), wsrc.data_ptr(), a.data_ptr(),
                             M, I, K, float(eps), grouped)
            return a
        if norm_scale is not None:
            x = self.rmsnorm(x, None, norm_scale, eps)
        g = self.linear(x, wsrc, None)
        if grouped:                                               # columns come out as [32 of z1 | the same 32 of z2] per block: back to [z1 | z2]
            g = g.view(M, I // 32, 2, 32).permute(0, 2, 1, 3).reshape(M, 2 * I).contiguous()
        return self.gelu_gate(g)

    def gelu_gate(self, g: torch.Tensor) -> torch.Tensor:
        self._need(g, torch.bfloat16, "gelu_gate g")
        M, I2 = g.shape
        a = torch.empty(M, I2 // 2, dtype=torch.bfloat16, device=g.device)
        with self._t("gelu_gate"):
            _check(self.lib.evo_gelu_gate_bf16(g.data_ptr(), a.data_ptr(), M, I2 // 2, _stream()),
                   "evo_gelu_gate_bf16")
        return a

    def logprob_entropy(self, logits: torch.Tensor, target: Optional[torch.Tensor], want_logprob=True,
                        want_entropy=False):
        """logits [M,V] bf16|f32, target [M] int64 -> (logprob [M] f32 | None, entropy [M] f32 | None)."""
        if logits.dtype not in (torch.bfloat16, torch.float32):
            raise RuntimeError(f"logprob logits: expected bf16 or f32, got {logits.dtype}")
        self._need(logits, logits.dtype, "logprob logits")
        M, V = logits.shape
        lp = torch.empty(M, dtype=torch.float32, device=logits.device) if want_logprob else None
        en = torch.empty(M, dtype=torch.float32, device=logits.device) if want_entropy else None
        if target is not None:
            target = target.reshape(-1).to(torch.int64).contiguous()
            if self.validate_ids and not torch.cuda.is_current_stream_capturing() and target.numel() \
                    and int(target.max().item()) >= V:
                raise IndexError(f"logprob target ids must be < {V} (negative = masked position)")
        _check(self.lib.evo_logprob_entropy(logits.data_ptr(), int(logits.dtype == torch.float32), _ptr(target),
                                            _ptr(lp), _ptr(en), M, V, _stream()),
               "evo_logprob_entropy")
        return lp, en


    def unembed_logprob_ok(self, h: torch.Tensor, emb: torch.Tensor) -> bool:
        return (h.is_cuda and h.dtype == torch.bfloat16 and emb.dtype == torch.bfloat16 and h.is_contiguous()
                and emb.is_contiguous() and emb.shape[0] == 512 and h.shape[1] % 32 == 0
                and os.environ.get("EVO_AMD_FUSED_TAIL", "1") != "0")

    def unembed_logprob(self, h: torch.Tensor, emb: torch.Tensor, target: Optional[torch.Tensor],
                        want_logprob=True, want_entropy=False):
        """Fused scoring tail: h [M,K] bf16 (final-norm output) x emb[512,K]^T -> (logprob [M] f32 | None,
        entropy [M] f32 | None) without materialising the [M, 512] logits."""
        self._need(h, torch.bfloat16, "unembed_logprob h")
        self._need(emb, torch.bfloat16, "unembed_logprob emb")
        M, K = h.shape
        V = emb.shape[0]
        lp = torch.empty(M, dtype=torch.float32, device=h.device) if want_logprob else None
        en = torch.empty(M, dtype=torch.float32, device=h.device) if want_entropy else None
        if target is not None:
            target = target.reshape(-1).to(torch.int64).contiguous()
            assert target.numel() == M
        with self._t("unembed_logprob"):
            _check(self.lib.evo_unembed_logprob_bf16(h.data_ptr(), emb.data_ptr(), _ptr(target), _ptr(lp), _ptr(en),
                                                     M, V, K, _stream()), "evo_unembed_logprob_bf16")
        return lp, en

    PROFILE_MAX_IDS = 8     # most vocabulary ids one profile launch takes (csrc/score_tail.hip ST_NSEL)

    @staticmethod
    def check_profile_ids(sel_ids, vocab: int = 512):
        """The ids of a profile as a list of ints: 1 .. PROFILE_MAX_IDS distinct values in [0, vocab) -- ValueError otherwise (host
        logic: what evo_unembed_profile_bf16 would answer with -1)."""
        try:
            ids = [int(i) for i in sel_ids]
            exact = all(i == j for i, j in zip(ids, sel_ids))
        except (TypeError, ValueError) as e:
            raise ValueError(f"profile ids: expected a sequence of integers, got {sel_ids!r}") from e
        if not exact:
            raise ValueError(f"profile ids: expected integers, got {list(sel_ids)!r}")
        if not 1 <= len(ids) <= HipOps.PROFILE_MAX_IDS:
            raise ValueError(f"profile ids: expected 1 to {HipOps.PROFILE_MAX_IDS} ids, got {len(ids)}")
        for i in ids:
            if not 0 <= i < vocab:
                raise ValueError(f"profile ids: id {i} is outside [0, {vocab})")
        if len(set(ids)) != len(ids):
            raise ValueError(f"profile ids: an id is given twice in {ids}")
        return ids

    def unembed_profile(self, h: torch.Tensor, emb: torch.Tensor, sel_ids, target: Optional[torch.Tensor] = None,
                        want_logprob=True, want_entropy=True):
        """Fused scoring tail with a profile: h [M,K] bf16 (final-norm output) x emb[512,K]^T -> (sel_logprob [M, n] f32 = the
        log-softmax at the n = len(sel_ids) chosen vocabulary ids of every row, logprob [M] f32 | None, entropy [M] f32 | None) in ONE
        launch, without materialising the [M, 512] logits; logprob / entropy are unembed_logprob's, bit for bit.  `sel_ids`: a host
        sequence of 1 .. 8 distinct ids in [0, 512) (ValueError otherwise)."""
        ids = self.check_profile_ids(sel_ids, emb.shape[0])
        self._need(h, torch.bfloat16, "unembed_profile h")
        self._need(emb, torch.bfloat16, "unembed_profile emb")
        if not self.unembed_logprob_ok(h, emb):
            raise RuntimeError("unembed_profile: the fused tail does not take these operands (unembed_logprob_ok)")
        M, K = h.shape
        V = emb.shape[0]
        sl = torch.empty(M, len(ids), dtype=torch.float32, device=h.device)
        lp = torch.empty(M, dtype=torch.float32, device=h.device) if want_logprob else None
        en = torch.empty(M, dtype=torch.float32, device=h.device) if want_entropy else None
        if target is not None:
            target = target.reshape(-1).to(torch.int64).contiguous()
            assert target.numel() == M
            self._need(target, torch.int64, "unembed_profile target")
        sel = (_c.c_int32 * len(ids))(*ids)                      # HOST array: read by the entry point at launch
        with self._t("unembed_profile"):
            _check(self.lib.evo_unembed_profile_bf16(h.data_ptr(), emb.data_ptr(), _ptr(target), sel, len(ids), sl.data_ptr(),
                                                     _ptr(lp), _ptr(en), M, V, K, _stream()), "evo_unembed_profile_bf16")
        return sl, lp, en

    POOL_MODES = {"mean": 0, "last": 1}
    POOL_WORKGROUPS = 1024      # strips of all sequences together: 4 per CU (16 waves) -- 1 x 131,073 and 8 x 8,193 both reach it

    def pool_rows(self, x: torch.Tensor, ranges, scale: Optional[torch.Tensor] = None, eps: float = 1e-6,
                  mode: str = "mean") -> torch.Tensor:
        """Masked row pooling (csrc/pool.hip): x [M, D] bf16 (row stride >= D), `ranges` = B pairs (first_row, n_rows) as a list or an
        int64 tensor [B, 2] -> [B, D] fp32: the mean (mode "mean") or the last row (mode "last") of each range, of x itself or -- with
        `scale` -- of the RMSNorm of its rows (scale * x / (rms(x) + eps), in fp32, no bf16 rounding)."""
        if not x.is_cuda or x.dtype != torch.bfloat16 or x.dim() != 2 or x.stride(1) != 1:
            raise RuntimeError("pool_rows: x must be a [M, D] bf16 device matrix with unit column stride")
        self._check_address(x.data_ptr(), "pool_rows x")
        if x.stride(0) % 8 or x.stride(0) < x.shape[1]:
            raise RuntimeError("pool_rows: x must have a row stride >= D that is a multiple of 8")
        if mode not in self.POOL_MODES:
            raise ValueError(f"pool_rows: mode must be one of {tuple(self.POOL_MODES)}, got {mode!r}")
        if scale is not None:
            self._need(scale, torch.bfloat16, "pool_rows scale")
            assert scale.numel() == x.shape[1]
        M, D = x.shape
        if isinstance(ranges, torch.Tensor):
            rg = ranges.to(device=x.device, dtype=torch.int64).reshape(-1, 2).contiguous()
            self._check_address(rg.data_ptr(), "pool_rows ranges", 8)
            longest = M
        else:
            pairs = [(int(a), int(n)) for a, n in ranges]
            for a, n in pairs:
                if a < 0 or n < 1 or a + n > M:
                    raise ValueError(f"pool_rows: range (first={a}, n={n}) is outside the {M} rows of x")
            rg = torch.tensor(pairs, dtype=torch.int64).reshape(-1, 2).to(x.device)
            longest = max(n for _, n in pairs) if pairs else 0
        B = rg.shape[0]
        if B < 1:
            raise ValueError("pool_rows: no ranges")
        # strips per sequence: POOL_WORKGROUPS over the batch, no strip below 16 rows (a wave then still pools 4 of them)
        n_strips = 1 if mode == "last" else max(1, min(-(-self.POOL_WORKGROUPS // B), -(-longest // 16)))
        ws = torch.empty(B * n_strips * D, dtype=torch.float32, device=x.device)
        out = torch.empty(B, D, dtype=torch.float32, device=x.device)
        with self._t("pool_rows"):
            _check(self.lib.evo_pool_rows_bf16(x.data_ptr(), M, D, x.stride(0), rg.data_ptr(), B, _ptr(scale), float(eps),
                                               self.POOL_MODES[mode], n_strips, ws.data_ptr(), out.data_ptr(), _stream()),
                   "evo_pool_rows_bf16")
        return out


    @staticmethod
    def pack_allow_mask(mask: torch.Tensor, device) -> torch.Tensor:
        """bool [512] -> the 64 device bytes `sample_rows` takes (bit j of byte b = token 8 b + j)."""
        m = torch.as_tensor(mask, dtype=torch.bool).reshape(-1).cpu()
        if m.numel() != 512 or not bool(m.any()):
            raise ValueError("allow mask: expected 512 flags with at least one set")
        w = (m.view(64, 8).to(torch.int32) << torch.arange(8, dtype=torch.int32)[None, :]).sum(-1)
        return w.to(torch.uint8).to(device)

    def sample_rows(self, logits: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor, temperature: torch.Tensor, seed: int,
                    stream: Optional[torch.Tensor] = None, count: Optional[torch.Tensor] = None, allow: Optional[torch.Tensor] = None,
                    active: Optional[torch.Tensor] = None, ids_out: Optional[torch.Tensor] = None,
                    logprob_out: Optional[torch.Tensor] = None, hist_ids: Optional[torch.Tensor] = None,
                    hist_logits: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """Seeded sampling on the device (csrc/sample.hip; specification: sh/sample.py sample_seeded): logits [S, 512] bf16 | f32 ->
        (ids [S] int64, logprob [S] f32 under the unfiltered log-softmax).  top_k int32 / top_p f32 / temperature f32 / stream int64 /
        count int64 / active bool are device tensors [S]; `allow` the 64 bytes of `pack_allow_mask`; `count` advances by one for
        every active row; with hist_ids [S, L] int64 / hist_logits [S, L, 512] f32 the token and the f32 row land at [s, count[s]].
        One launch on the current stream, nothing read back: capturable."""
        if logits.dtype not in (torch.bfloat16, torch.float32) or logits.dim() != 2 or not logits.is_cuda:
            raise RuntimeError("sample_rows: logits must be a [S, 512] bf16 or f32 device matrix")
        S, V = logits.shape
        if logits.stride(1) != 1 or logits.stride(0) % 8 or logits.stride(0) < V or logits.data_ptr() % 16:
            logits = logits.contiguous()
        dev = logits.device

        def need(t, dtype, shape, what):
            if t is not None and (t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev):
                raise RuntimeError(f"sample_rows: {what} must be a contiguous {dtype} tensor of shape {shape} on {dev}")
        need(top_k, torch.int32, (S,), "top_k")
        need(top_p, torch.float32, (S,), "top_p")
        need(temperature, torch.float32, (S,), "temperature")
        need(stream, torch.int64, (S,), "stream")
        need(count, torch.int64, (S,), "count")
        need(active, torch.bool, (S,), "active")
        need(allow, torch.uint8, (64,), "allow")
        if ids_out is None:
            ids_out = torch.empty(S, dtype=torch.int64, device=dev)
        if logprob_out is None:
            logprob_out = torch.empty(S, dtype=torch.float32, device=dev)
        need(ids_out.view(-1), torch.int64, (S,), "ids_out")
        need(logprob_out, torch.float32, (S,), "logprob_out")
        hist_len = 0
        if hist_ids is not None or hist_logits is not None:
            if count is None:
                raise RuntimeError("sample_rows: a history needs the per-row count")
            hist_len = int(hist_ids.shape[1] if hist_ids is not None else hist_logits.shape[1])
            need(hist_ids, torch.int64, (S, hist_len), "hist_ids")
            need(hist_logits, torch.float32, (S, hist_len, V), "hist_logits")
        with self._t("sample_rows"):
            _check(self.lib.evo_sample_rows_f32(logits.data_ptr(), int(logits.dtype == torch.float32), logits.stride(0), top_k.data_ptr(),
                                                top_p.data_ptr(), temperature.data_ptr(), _ptr(allow), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                                _ptr(stream), _ptr(count), _ptr(active), ids_out.data_ptr(), logprob_out.data_ptr(),
                                                _ptr(hist_ids), _ptr(hist_logits), hist_len, S, V, _stream()), "evo_sample_rows_f32")
        return ids_out, logprob_out

    @staticmethod
    def pack_stop_sequences(patterns) -> Tuple[torch.Tensor, torch.Tensor]:
        """Stop patterns as id lists (at most 8 of 1 to 8 tokens) -> (int32 [n_seq, 8], int32 [n_seq]) HOST tensors: `sample_rows_ctl`
        hands them to the launch by value."""
        from .sh.sample import pack_stop_sequences
        return pack_stop_sequences(patterns)

    def sample_rows_ctl(self, logits: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor, temperature: torch.Tensor, seed: int,
                        count: torch.Tensor, active: torch.Tensor, limit: torch.Tensor, length: torch.Tensor, finish: torch.Tensor,
                        stream: Optional[torch.Tensor] = None, allow: Optional[torch.Tensor] = None,
                        ids_out: Optional[torch.Tensor] = None, logprob_out: Optional[torch.Tensor] = None,
                        hist_ids: Optional[torch.Tensor] = None, hist_logits: Optional[torch.Tensor] = None,
                        hist_logprob: Optional[torch.Tensor] = None, stop_mask: Optional[torch.Tensor] = None, stop_seq=None,
                        stop_frame: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
        """`sample_rows` with job control (csrc/sample.hip; specification: sh/sample.py finish_reason / sample_ctl): the same draw, then the
        row ends its own job -- a token of `stop_mask` (64 bytes of `pack_allow_mask`), an in-frame stop pattern (`stop_seq`: the pair of
        `pack_stop_sequences`) at the end of its recorded tokens, or `limit` [S] int64 reached -- by clearing its byte of `active` [S] bool
        and writing `length` [S] int64 and `finish` [S] uint8 (1 stop token, 2 stop sequence, 3 length).  hist_ids [S, L] int64,
        hist_logits [S, L, 512] f32 and hist_logprob [S, L] f32 are each optional.  One launch, nothing read back: capturable."""
        return self._sample_rows_ctl("sample_rows_ctl", "evo_sample_rows_ctl_f32", None, logits, top_k, top_p, temperature, seed, count, active,
                                     limit, length, finish, stream, allow, ids_out, logprob_out, hist_ids, hist_logits, hist_logprob,
                                     stop_mask, stop_seq, stop_frame)

    def sample_rows_dfa(self, logits: torch.Tensor, top_k: torch.Tensor, top_p: torch.Tensor, temperature: torch.Tensor, seed: int,
                        count: torch.Tensor, active: torch.Tensor, limit: torch.Tensor, length: torch.Tensor, finish: torch.Tensor,
                        dfa_alphabet: torch.Tensor, dfa_next: torch.Tensor, dfa_base: torch.Tensor, dfa_state: torch.Tensor,
                        stream: Optional[torch.Tensor] = None, allow: Optional[torch.Tensor] = None,
                        ids_out: Optional[torch.Tensor] = None, logprob_out: Optional[torch.Tensor] = None,
                        hist_ids: Optional[torch.Tensor] = None, hist_logits: Optional[torch.Tensor] = None,
                        hist_logprob: Optional[torch.Tensor] = None, stop_mask: Optional[torch.Tensor] = None, stop_seq=None,
                        stop_frame: int = 1) -> Tuple[torch.Tensor, torch.Tensor]:
        """`sample_rows_ctl` under a per-row token automaton (csrc/sample.hip; specification: sh/sample.py sample_dfa).
        `dfa_alphabet`: HOST int32 [1 ... 8] distinct token ids; `dfa_next`: device int32 [n_states, 8] (>= 0 next state relative to the
        row's base, -2 accept, other negative values forbidden); `dfa_base` [S] device int64 (the table row of the row's state 0; < 0: the row
        is unconstrained); `dfa_state` [S] device int32, in/out.  A row draws from the tokens its state permits (and `allow`), the token moves
        its state; finish 4 = the constraint is complete, 5 = a dead end (nothing drawn).  One launch, nothing read back: capturable."""
        return self._sample_rows_ctl("sample_rows_dfa", "evo_sample_rows_dfa_f32", (dfa_alphabet, dfa_next, dfa_base, dfa_state), logits, top_k,
                                     top_p, temperature, seed, count, active, limit, length, finish, stream, allow, ids_out, logprob_out,
                                     hist_ids, hist_logits, hist_logprob, stop_mask, stop_seq, stop_frame)

    def _sample_rows_ctl(self, me, entry, dfa, logits, top_k, top_p, temperature, seed, count, active, limit, length, finish, stream, allow,
                         ids_out, logprob_out, hist_ids, hist_logits, hist_logprob, stop_mask, stop_seq, stop_frame):
        """The argument checks and the call of both control entries (`dfa`: None, or the four automaton operands of `sample_rows_dfa`)."""
        if logits.dtype not in (torch.bfloat16, torch.float32) or logits.dim() != 2 or not logits.is_cuda:
            raise RuntimeError(f"{me}: logits must be a [S, 512] bf16 or f32 device matrix")
        S, V = logits.shape
        if logits.stride(1) != 1 or logits.stride(0) % 8 or logits.stride(0) < V or logits.data_ptr() % 16:
            logits = logits.contiguous()
        dev = logits.device

        def need(t, dtype, shape, what, required=False):
            if t is None and not required:
                return
            if t is None or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
                raise RuntimeError(f"{me}: {what} must be a contiguous {dtype} tensor of shape {shape} on {dev}")
        need(top_k, torch.int32, (S,), "top_k", True)
        need(top_p, torch.float32, (S,), "top_p", True)
        need(temperature, torch.float32, (S,), "temperature", True)
        need(stream, torch.int64, (S,), "stream")
        need(count, torch.int64, (S,), "count", True)
        need(active, torch.bool, (S,), "active", True)
        need(limit, torch.int64, (S,), "limit", True)
        need(length, torch.int64, (S,), "length", True)
        need(finish, torch.uint8, (S,), "finish", True)
        need(allow, torch.uint8, (64,), "allow")
        need(stop_mask, torch.uint8, (64,), "stop_mask")
        if ids_out is None:
            ids_out = torch.empty(S, dtype=torch.int64, device=dev)
        if logprob_out is None:
            logprob_out = torch.empty(S, dtype=torch.float32, device=dev)
        need(ids_out.view(-1), torch.int64, (S,), "ids_out")
        need(logprob_out, torch.float32, (S,), "logprob_out")
        hist_len = 0
        for h in (hist_ids, hist_logits, hist_logprob):
            if h is not None:
                hist_len = int(h.shape[1])
        if hist_len:
            need(hist_ids, torch.int64, (S, hist_len), "hist_ids")
            need(hist_logits, torch.float32, (S, hist_len, V), "hist_logits")
            need(hist_logprob, torch.float32, (S, hist_len), "hist_logprob")
        seq_ptr = len_ptr = None
        n_seq = 0
        if stop_seq is not None and len(stop_seq[1]):
            seq, seq_len = stop_seq
            if seq.dtype != torch.int32 or seq_len.dtype != torch.int32 or seq.is_cuda or seq_len.is_cuda or not seq.is_contiguous() \
                    or tuple(seq.shape) != (seq_len.numel(), 8):
                raise RuntimeError(f"{me}: stop_seq must be the host pair of pack_stop_sequences")
            if hist_ids is None:
                raise RuntimeError(f"{me}: stop sequences need hist_ids")
            n_seq, seq_ptr, len_ptr = int(seq_len.numel()), seq.data_ptr(), seq_len.data_ptr()
        extra = ()
        if dfa is not None:
            alphabet, nxt, base, state = dfa
            if not isinstance(alphabet, torch.Tensor) or alphabet.dtype != torch.int32 or alphabet.is_cuda or alphabet.dim() != 1 \
                    or not alphabet.is_contiguous() or not 1 <= alphabet.numel() <= 8:
                raise RuntimeError(f"{me}: dfa_alphabet must be a host int32 vector of 1 to 8 token ids")
            ids = alphabet.tolist()
            if len(set(ids)) != len(ids) or any(not 0 <= t < 512 for t in ids):
                raise RuntimeError(f"{me}: dfa_alphabet must hold distinct token ids in [0, 512)")
            if not isinstance(nxt, torch.Tensor) or nxt.dim() != 2 or not 1 <= nxt.shape[0] <= 1 << 27 or nxt.data_ptr() % 16:
                raise RuntimeError(f"{me}: dfa_next must be a 16-byte aligned [n_states, 8] matrix of 1 to 2^27 states")
            need(nxt, torch.int32, (nxt.shape[0], 8), "dfa_next", True)
            need(base, torch.int64, (S,), "dfa_base", True)
            need(state, torch.int32, (S,), "dfa_state", True)
            extra = (alphabet.data_ptr(), int(alphabet.numel()), nxt.data_ptr(), int(nxt.shape[0]), base.data_ptr(), state.data_ptr())
        with self._t(me):
            _check(getattr(self.lib, entry)(
                logits.data_ptr(), int(logits.dtype == torch.float32), logits.stride(0), top_k.data_ptr(), top_p.data_ptr(),
                temperature.data_ptr(), _ptr(allow), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(stream), count.data_ptr(), active.data_ptr(),
                ids_out.data_ptr(), logprob_out.data_ptr(), _ptr(hist_ids), _ptr(hist_logits), _ptr(hist_logprob), hist_len,
                limit.data_ptr(), _ptr(stop_mask), seq_ptr, len_ptr, n_seq, int(stop_frame), length.data_ptr(), finish.data_ptr(), *extra,
                S, V, _stream()), entry)
        return ids_out, logprob_out

    # ---- k-mer repeat control: the optional group "repeat" (csrc/repeat.hip) ------------------------------------------
    def repeat_rows(self, logits: torch.Tensor, out: torch.Tensor, active: torch.Tensor, counts: torch.Tensor, ctx: torch.Tensor,
                    stat: torch.Tensor, levels: torch.Tensor, alphabet: torch.Tensor, k: int, fed_ids: Optional[torch.Tensor] = None,
                    end_num: Optional[torch.Tensor] = None, end_min_tokens: int = 1, count: Optional[torch.Tensor] = None,
                    length: Optional[torch.Tensor] = None, finish: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The launch in front of the job-control sampler launch (specification: sh/sample.py repeat_row): logits [S, 512] bf16 | f32 ->
        `out` [S, 512] f32, the row the sampler draws from.  Per row with `active` [S] bool set: the token `fed_ids` [S] (or [S, 1]) int64
        is folded into `counts` [S, M] int32, `ctx` [S, 2] int32 and `stat` [S, 2] int64 (None: nothing is folded); with `end_num` [S]
        int32 the rule may end the job (active cleared, length[s] = count[s], finish[s] = 6, the row of `out` left alone); otherwise the
        row is widened and levels[s][min(c, 7)] (`levels` [S, 8] f32) is subtracted on every symbol of `alphabet` (HOST int32, 1 ... 8
        distinct ids), c the count of the k-mer it would complete.  M = len(alphabet) ** k.  One launch, nothing read back: capturable."""
        me = "repeat_rows"
        if logits.dtype not in (torch.bfloat16, torch.float32) or logits.dim() != 2 or not logits.is_cuda:
            raise RuntimeError(f"{me}: logits must be a [S, 512] bf16 or f32 device matrix")
        S, V = logits.shape
        if logits.stride(1) != 1 or logits.stride(0) % 8 or logits.stride(0) < V or logits.data_ptr() % 16:
            logits = logits.contiguous()
        dev = logits.device
        if not isinstance(alphabet, torch.Tensor) or alphabet.dtype != torch.int32 or alphabet.is_cuda or alphabet.dim() != 1 \
                or not alphabet.is_contiguous() or not 1 <= alphabet.numel() <= 8:
            raise RuntimeError(f"{me}: alphabet must be a host int32 vector of 1 to 8 token ids")
        ids = alphabet.tolist()
        if len(set(ids)) != len(ids) or any(not 0 <= t < 512 for t in ids):
            raise RuntimeError(f"{me}: alphabet must hold distinct token ids in [0, 512)")
        n_sym, k = len(ids), int(k)
        if k < 1 or (n_sym > 1 and (k > 20 or n_sym ** k > 1 << 20)):
            raise RuntimeError(f"{me}: k = {k} over {n_sym} symbols is outside 1 <= n_sym ** k <= 2^20")
        M = n_sym ** k if n_sym > 1 else 1

        def need(t, dtype, shape, what, required=False):
            if t is None and not required:
                return
            if t is None or t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous() or t.device != dev:
                raise RuntimeError(f"{me}: {what} must be a contiguous {dtype} tensor of shape {shape} on {dev}")
        need(out, torch.float32, (S, V), "out", True)
        if out.data_ptr() % 16:
            raise RuntimeError(f"{me}: out must be 16-byte aligned")
        need(active, torch.bool, (S,), "active", True)
        need(counts, torch.int32, (S, M), "counts", True)
        need(ctx, torch.int32, (S, 2), "ctx", True)
        need(stat, torch.int64, (S, 2), "stat", True)
        need(levels, torch.float32, (S, 8), "levels", True)
        need(None if fed_ids is None else fed_ids.view(-1), torch.int64, (S,), "fed_ids")
        need(end_num, torch.int32, (S,), "end_num")
        armed = end_num is not None
        need(count, torch.int64, (S,), "count", armed)
        need(length, torch.int64, (S,), "length", armed)
        need(finish, torch.uint8, (S,), "finish", armed)
        if armed and int(end_min_tokens) < 1:
            raise RuntimeError(f"{me}: end_min_tokens must be >= 1")
        with self._t(me):
            _check(self.lib.evo_repeat_rows_f32(logits.data_ptr(), int(logits.dtype == torch.float32), logits.stride(0), out.data_ptr(),
                                                _ptr(fed_ids), active.data_ptr(), counts.data_ptr(), ctx.data_ptr(), stat.data_ptr(),
                                                levels.data_ptr(), _ptr(end_num), int(end_min_tokens), _ptr(count), _ptr(length),
                                                _ptr(finish), alphabet.data_ptr(), n_sym, k, M, S, V, _stream()), "evo_repeat_rows_f32")
        return out

    # ---- beam search: the optional group "beam" (csrc/beam.hip) ---------------------------------------------------------
    def beam_select(self, logits: torch.Tensor, cum: torch.Tensor, ended: torch.Tensor, length: torch.Tensor, ids: torch.Tensor,
                    parent: torch.Tensor, beam_width: int, group_active: Optional[torch.Tensor] = None, allow: Optional[torch.Tensor] = None,
                    stop_mask: Optional[torch.Tensor] = None, hist_parent: Optional[torch.Tensor] = None,
                    hist_ids: Optional[torch.Tensor] = None, hist_cum: Optional[torch.Tensor] = None, step: Optional[torch.Tensor] = None,
                    t: int = -1) -> None:
        """One step of beam search on the device (specification: sh/sample.py beam_select): logits [S, 512] bf16 | f32; per-slot state, in
        place: cum [S] f32, ended [S] uint8 | bool, length [S] int64, ids [S] (or [S, 1]) int64; parent [S] int64 out.  Groups of
        `beam_width` consecutive slots; group_active [S // beam_width] uint8 | bool; `allow` / `stop_mask`: the 64 bytes of
        `pack_allow_mask`.  History [S, L]: hist_parent int32, hist_ids int64, hist_cum f32 (optional), written at column step[g] (`step`:
        int64 [S // beam_width], advanced by the launch) or at the scalar `t`.  One launch, nothing read back: capturable."""
        if logits.dtype not in (torch.bfloat16, torch.float32) or logits.dim() != 2 or not logits.is_cuda:
            raise RuntimeError("beam_select: logits must be a [S, 512] bf16 or f32 device matrix")
        S, V = logits.shape
        W = int(beam_width)
        if not 1 <= W <= 8 or S < W:
            raise RuntimeError(f"beam_select: beam_width {W} must be 1 ... 8 and at most S = {S}")
        if logits.stride(1) != 1 or logits.stride(0) % 8 or logits.stride(0) < V or logits.data_ptr() % 16:
            logits = logits.contiguous()
        dev, G = logits.device, S // W

        def need(x, dtypes, shape, what, required=False):
            if x is None and not required:
                return
            if x is None or x.dtype not in dtypes or tuple(x.shape) != shape or not x.is_contiguous() or x.device != dev:
                raise RuntimeError(f"beam_select: {what} must be a contiguous {dtypes[0]} tensor of shape {shape} on {dev}")
        bytes_ = (torch.uint8, torch.bool)
        need(cum, (torch.float32,), (S,), "cum", True)
        need(ended, bytes_, (S,), "ended", True)
        need(length, (torch.int64,), (S,), "length", True)
        need(ids.view(-1), (torch.int64,), (S,), "ids", True)
        need(parent, (torch.int64,), (S,), "parent", True)
        need(group_active, bytes_, (G,), "group_active")
        need(allow, (torch.uint8,), (64,), "allow")
        need(stop_mask, (torch.uint8,), (64,), "stop_mask")
        need(step, (torch.int64,), (G,), "step")
        hist_len = 0
        if step is not None or int(t) >= 0:
            if hist_parent is None or hist_ids is None:
                raise RuntimeError("beam_select: a step to record needs hist_parent and hist_ids")
            hist_len = int(hist_parent.shape[1])
            need(hist_parent, (torch.int32,), (S, hist_len), "hist_parent")
            need(hist_ids, (torch.int64,), (S, hist_len), "hist_ids")
            need(hist_cum, (torch.float32,), (S, hist_len), "hist_cum")
        with self._t("beam_select"):
            _check(self.lib.evo_beam_select_f32(logits.data_ptr(), int(logits.dtype == torch.float32), logits.stride(0), _ptr(allow),
                                                _ptr(stop_mask), _ptr(group_active), cum.data_ptr(), ended.data_ptr(), length.data_ptr(),
                                                ids.data_ptr(), parent.data_ptr(), _ptr(hist_parent), _ptr(hist_ids), _ptr(hist_cum), hist_len,
                                                _ptr(step), int(t), W, S, V, _stream()), "evo_beam_select_f32")

    def gather_table(self, fixed, per_token=()):
        """Registers the tensors `gather_rows` moves: `fixed` [S, ...] whose whole rows move, `per_token` [S, n_tokens, ...] of which only
        the first own_pos[parent] + 1 tokens move.  -> a `GatherTable` (the device table, the scratch buffer of S rows, its sizes)."""
        tensors = [(x, False) for x in fixed] + [(x, True) for x in per_token]
        if not tensors:
            raise RuntimeError("gather_table: nothing to register")
        S, dev = int(tensors[0][0].shape[0]), tensors[0][0].device
        rows, off, max_row = [], 0, 0
        for x, tok in tensors:
            if not x.is_cuda or x.device != dev or x.shape[0] != S or x.dim() < (3 if tok else 2) or not x[0].is_contiguous():
                raise RuntimeError("gather_table: every tensor is [S, ...] on one ROCm device with contiguous rows")
            es = x.element_size()
            stride, row = x.stride(0) * es, x[0].numel() * es
            bpt = x[0, 0].numel() * es if tok else 0
            if x.data_ptr() % 16 or stride % 16 or row % 16 or bpt % 16 or row < 16 or stride < row:
                raise RuntimeError("gather_table: addresses, row strides, rows and tokens must be multiples of 16 bytes")
            rows.append([x.data_ptr(), stride, row, bpt, off, 0])
            off += row
            max_row = max(max_row, row)
        if S > 65535 or len(rows) > 65535:
            raise RuntimeError("gather_table: at most 65535 slots and 65535 tensors")
        return GatherTable(table=torch.tensor(rows, dtype=torch.int64).to(dev), scratch=torch.empty(S * off, dtype=torch.uint8, device=dev),
                           row_bytes=off, max_row_bytes=max_row, n_slots=S, tensors=[x for x, _ in tensors])

    def gather_rows(self, tab: "GatherTable", parent: torch.Tensor, own_pos: torch.Tensor) -> None:
        """The reparenting copy (csrc/beam.hip): for every slot s with parent[s] != s, row parent[s] of every tensor of `tab` goes to row
        s -- out to the scratch buffer in one launch, back in a second.  parent / own_pos: device int64 [S].  Capturable."""
        S = tab.n_slots
        for x, what in ((parent, "parent"), (own_pos, "own_pos")):
            if x.dtype != torch.int64 or tuple(x.shape) != (S,) or not x.is_contiguous() or x.device != tab.table.device:
                raise RuntimeError(f"gather_rows: {what} must be a contiguous int64 tensor of shape ({S},) on {tab.table.device}")
        with self._t("gather_rows"):
            for back in (0, 1):
                _check(self.lib.evo_gather_rows(tab.table.data_ptr(), int(tab.table.shape[0]), parent.data_ptr(), own_pos.data_ptr(),
                                                tab.scratch.data_ptr(), tab.row_bytes, tab.max_row_bytes, S, back, _stream()),
                       "evo_gather_rows")


class GatherTable:
    """What `HipOps.gather_table` registers: table int64 [n, 6] on the device (include/evo_mi355x.h: evo_gather_rows), the scratch buffer
    [S x row_bytes] bytes, and the tensors themselves (kept alive: the table holds their addresses)."""

    def __init__(self, table, scratch, row_bytes, max_row_bytes, n_slots, tensors):
        self.table, self.scratch, self.row_bytes, self.max_row_bytes, self.n_slots, self.tensors = \
            table, scratch, int(row_bytes), int(max_row_bytes), int(n_slots), tensors

    @property
    def scratch_bytes(self) -> int:
        return int(self.scratch.numel())


_DEFAULT_OPS = None


def default_ops() -> HipOps:
    global _DEFAULT_OPS
    if _DEFAULT_OPS is None:
        _DEFAULT_OPS = HipOps()
    return _DEFAULT_OPS
