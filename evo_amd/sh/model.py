"""`stripedhyena.model.StripedHyena` mirror: the host side of the MI355X-native forward engine.

The class keeps the contract evo consumes [REF evo/models.py:146-150; evo/scoring.py:81;
evo/generation.py:105-155]:
    model = StripedHyena(config); model.load_state_dict(sd, strict=True)
    model.to_bfloat16_except_poles_residues(); model.to(device)
    logits, cache = model(input_ids, inference_params_dict=None, padding_mask=None)
    cache = model.initialize_inference_params()
with the state-dict key set of SURVEY.md section B.  All arithmetic is dispatched to an `ops` object:
`evo_amd.ops.HipOps` (hand-written gfx950 kernels over the C ABI, the dense layers included) in the product.
There is no CPU fallback here: with no `ops` injected and no usable HIP library the first forward raises.
(`tests/` inject an oracle-backed ops object to exercise this host logic on CPU.)
"""
from __future__ import annotations

import contextlib
import math
import weakref
from typing import Dict, List, Optional, Tuple

import torch
import torch.nn as nn

from ..backend import Backend                            # (the contract of `ops`, and the pure host rules every backend shares)
from .cache import (ROWINV_SPLITS, W8_MAX_ROWS, W8_WIDE_K, Fp8KV, InferenceParams, PagedKV, RecurrentInferenceParams, check_kv_dtype, check_rowinv_rows, check_weight_dtype,
                    check_weight_rows)
from .utils import dotdict


@contextlib.contextmanager
def capture_graph(graph):
    """`torch.cuda.graph(graph)` whose capture BEGINS outside inference mode, whatever mode the caller is in (decode steps run under
    inference mode; the body of the `with` stays in the caller's mode).  torch creates the capture state of its random generator with the
    first live graph, in the mode capture_begin runs in, and keeps it while any graph lives: created under inference mode it is an
    inference tensor, and every later capture outside inference mode, anywhere in the process, fails on its in-place update for as long
    as that graph lives.  Created here it is an ordinary tensor, which either mode may update.  Every capture of this package (the decode
    graph below, the decode pool's step) goes through here, so that they agree."""
    with contextlib.ExitStack() as stack:
        with torch.inference_mode(False):
            stack.enter_context(torch.cuda.graph(graph))
        yield


def _cfg(config, key, default):
    v = config.get(key, None) if isinstance(config, dict) else getattr(config, key, None)
    return default if v is None else v


class _Params(nn.Module):
    """A bag of named parameters (keeps the upstream module/parameter names for state-dict parity)."""

    def __init__(self, **shapes):
        super().__init__()
        for name, (shape, dtype) in shapes.items():
            self.register_parameter(name, nn.Parameter(torch.empty(*shape, dtype=dtype), requires_grad=False))


class _MLP(nn.Module):
    def __init__(self, D, inner):
        super().__init__()
        bf = torch.bfloat16
        self.l1 = _Params(weight=((inner, D), bf))
        self.l2 = _Params(weight=((inner, D), bf))
        self.l3 = _Params(weight=((D, inner), bf))


class _HyenaBlock(nn.Module):
    """ParallelGatedConvBlock parameters."""

    def __init__(self, D, inner, state_size, filt_len):
        super().__init__()
        bf = torch.bfloat16
        self.pre_norm = _Params(scale=((D,), bf))
        self.post_norm = _Params(scale=((D,), bf))
        self.projections = _Params(weight=((3 * D, D), bf), bias=((3 * D,), bf))
        self.filter = _Params(short_filter_weight=((3 * D, 1, filt_len), bf), short_filter_bias=((3 * D,), bf),
                              D=((D,), bf), poles=((D, state_size, 1, 2), torch.float32),
                              residues=((D, state_size, 1, 2), torch.float32))
        self.out_filter_dense = _Params(weight=((D, D), bf), bias=((D,), bf))
        self.mlp = _MLP(D, inner)


class _MHA(nn.Module):
    def __init__(self, D, hd):
        super().__init__()
        bf = torch.bfloat16
        self.Wqkv = _Params(weight=((3 * D, D), bf), bias=((3 * D,), bf))
        self.out_proj = _Params(weight=((D, D), bf), bias=((D,), bf))
        self.rotary_emb = nn.Module()
        self.rotary_emb.register_buffer("inv_freq", torch.empty(hd // 2, dtype=torch.float32), persistent=True)


class _AttentionBlock(nn.Module):
    def __init__(self, D, inner, hd):
        super().__init__()
        bf = torch.bfloat16
        self.pre_norm = _Params(scale=((D,), bf))
        self.post_norm = _Params(scale=((D,), bf))
        self.inner_mha_cls = _MHA(D, hd)
        self.mlp = _MLP(D, inner)


class _Unembed(nn.Module):
    """The tied unembedding (`weight` is embedding_layer.weight).  `unembed(u)` [..., D] -> logits [..., V], the API of upstream's
    VocabParallelEmbedding.unembed -- so a caller can reach the logits of a hidden state, and the identity-unembed recipe (replace
    `model.unembed` by a module whose unembed() returns its input) finds the method it overrides."""

    def __init__(self, owner, weight):
        super().__init__()
        self.weight = weight
        object.__setattr__(self, "_owner", weakref.ref(owner))     # (not a submodule: no cycle in the module tree)

    def unembed(self, u: torch.Tensor) -> torch.Tensor:
        owner = self._owner()
        if owner is not None:
            ops = owner.ops
        else:
            from ..ops import default_ops
            ops = default_ops()
        D = u.shape[-1]
        return ops.linear(u.reshape(-1, D).contiguous(), self.weight, None).view(*u.shape[:-1], self.weight.shape[0])


class StripedHyena(nn.Module):
    def __init__(self, config, ops=None):
        super().__init__()
        if not isinstance(config, dict):
            raise TypeError("config must be a dict / dotdict")
        self.config = config if isinstance(config, dotdict) else dotdict(config)
        c = self.config
        self.vocab_size = int(_cfg(c, "vocab_size", 512))
        self.hidden_size = D = int(_cfg(c, "hidden_size", 4096))
        self.num_layers = int(_cfg(c, "num_layers", 32))
        self.attn_layer_idxs = list(_cfg(c, "attn_layer_idxs", [8, 16, 24]))
        self.hyena_layer_idxs = list(_cfg(c, "hyena_layer_idxs",
                                          [i for i in range(self.num_layers) if i not in self.attn_layer_idxs]))
        self.num_heads = int(_cfg(c, "num_attention_heads", 32))
        self.head_dim = D // self.num_heads
        self.state_size = int(_cfg(c, "state_size", 8))
        self.short_filter_length = int(_cfg(c, "short_filter_length", 3))
        self.eps = float(_cfg(c, "eps", 1e-6))
        mult = int(_cfg(c, "inner_size_multiple_of", 16))
        inner = _cfg(c, "inner_mlp_size", None)
        if inner is None:
            inner = mult * ((int(2 * D * 4 / 3) + mult - 1) // mult)
        self.inner_size = int(inner)
        self.rotary_base = float(_cfg(c, "rotary_emb_base", 10000.0))
        self.rotary_scaling = float(_cfg(c, "rotary_emb_scaling_factor", 1.0)) \
            if bool(_cfg(c, "use_interpolated_rotary_pos_emb", False)) else 1.0
        self.max_seqlen = int(_cfg(c, "max_seqlen", 8192))
        if self.state_size != 8 or self.short_filter_length != 3:
            raise ValueError("the gfx950 Hyena kernels are built for state_size 8 and short_filter_length 3")

        bf = torch.bfloat16
        self.embedding_layer = _Params(weight=((self.vocab_size, D), bf))
        self.norm = _Params(scale=((D,), bf)) if bool(_cfg(c, "final_norm", True)) else None
        self.unembed = _Unembed(self, self.embedding_layer.weight)  # tied [REF evo/models.py:132-137]
        blocks = []
        for i in range(self.num_layers):
            if i in self.attn_layer_idxs:
                blocks.append(_AttentionBlock(D, self.inner_size, self.head_dim))
            else:
                blocks.append(_HyenaBlock(D, self.inner_size, self.state_size, self.short_filter_length))
        self.blocks = nn.ModuleList(blocks)
        self._ops = Backend.adopt(ops)
        self._packed = False
        self._rot_cache: Dict[Tuple[int, int, str], Tuple[torch.Tensor, torch.Tensor]] = {}
        self._norms_folded = False                                 # fold_norms_: ONE weight set, the parameters are the folded weights
        self._dgraph = self._dgraph_warm = None                    # the captured decode step and the caches whose first step ran eagerly
        self._w8 = None                                            # the FP8 copies of the decode step's dense weights (prepare_fp8_weights)
        self.decode_graph_replays = 0
        self._tail_ix = self._rows = self._inv_freq_dev = None     # small index tensors: _tail_split_index, _row_index, _inv_freq
        # debugging / parity hook: a list that receives the residual stream entering every block, or only the listed ones (num_layers = the final stream)
        self.block_taps = self.block_tap_idxs = None

    # ------------------------------------------------------------------ state-dict / dtype / device
    def load_state_dict(self, state_dict, strict: bool = True, assign: bool = True):
        """Strict key/shape check, then ADOPT the given tensors (no 13 GB copy)."""
        own = dict(self.named_parameters(remove_duplicate=False))
        own.update(dict(self.named_buffers(remove_duplicate=False)))
        missing = [k for k in own if k not in state_dict]
        unexpected = [k for k in state_dict if k not in own]
        if "unembed.weight" in missing and "embedding_layer.weight" in state_dict:
            missing.remove("unembed.weight")
        if strict and (missing or unexpected):
            raise RuntimeError(f"Error(s) in loading state_dict for StripedHyena: missing keys {missing}, "
                               f"unexpected keys {unexpected}")
        if self._norms_folded:
            raise RuntimeError("load_state_dict on a model that holds one folded weight set (fold_norms_): build a fresh StripedHyena")
        for k, t in state_dict.items():
            if k not in own or k == "unembed.weight":
                continue
            if tuple(own[k].shape) != tuple(t.shape):
                raise RuntimeError(f"size mismatch for {k}: checkpoint {tuple(t.shape)} vs model {tuple(own[k].shape)}")
            own[k].data = t.detach()
        self._packed = False
        self._w8 = None
        self._rot_cache.clear()
        from torch.nn.modules.module import _IncompatibleKeys
        return _IncompatibleKeys(missing, unexpected)

    def to_bfloat16_except_poles_residues(self):
        """bf16 everywhere except the fp32 poles / residues (and inv_freq) [REF evo/models.py:148]."""
        for k, p in self.named_parameters():
            if k.endswith("poles") or k.endswith("residues"):
                p.data = p.data.to(torch.float32)
            else:
                p.data = p.data.to(torch.bfloat16)
        for _, b in self.named_buffers():
            b.data = b.data.to(torch.float32)
        self._packed = False
        self._w8 = None

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        self._packed = False
        self._w8 = None
        self._rot_cache.clear()
        return out

    @property
    def device(self):
        return self.embedding_layer.weight.device

    @property
    def ops(self):
        if self._ops is None:
            from ..ops import default_ops
            self._ops = default_ops()          # raises if the HIP library / GPU is unavailable
        return self._ops

    def _pack(self):
        if self._norms_folded:
            raise RuntimeError("this StripedHyena holds ONE folded weight set (fold_norms_): its derived tensors cannot be rebuilt from the "
                               "parameters -- moving / re-typing / re-loading needs a fresh model")
        self._pack_impl()

    def _pack_impl(self):
        """Derived device-side layouts: fused [l1;l2] weight (one GEMM for the gated MLP) with the inner size
        zero-padded to a multiple of 256 (10928 -> 11008: hipBLASLt runs the l3 GEMM, K = inner, 14 % faster
        without a K tail and the fused l1|l2 GEMM 3 % faster; the padded rows/columns are exact zeros, so
        gelu(0)*0 = 0 flows through and the result is bit-identical), contiguous [3D,3] FIR taps and [D,8,2]
        poles/residues.  l1/l2/l3 keep their state-dict entries as views of the padded buffers."""
        self._w8 = None                                       # (an FP8 set quantised the buffers replaced here)
        for blk in self.blocks:
            l1, l2, l3 = blk.mlp.l1.weight, blk.mlp.l2.weight, blk.mlp.l3.weight
            inner, D_ = l1.shape
            ipad = ((inner + 255) // 256) * 256 if inner >= 1024 else inner
            w12 = l1.data.new_zeros(2 * ipad, D_)
            w12[:inner] = l1.data
            w12[ipad:ipad + inner] = l2.data
            w3 = l3.data.new_zeros(D_, ipad)
            w3[:, :inner] = l3.data
            l1.data = w12[:inner]
            l2.data = w12[ipad:ipad + inner]
            l3.data = w3[:, :inner]
            blk.mlp._w12 = w12
            blk.mlp._w3 = w3
            # the same rows regrouped for the one-launch gated form of the prefill path (GELU * gate in the dense layer's epilogue:
            # csrc/gemm.hip) are a copy (180 MB per layer at D = 4096: 5.8 GB for 32 layers; the decode kernels stream `w12` as it is):
            # built on the first prefill-sized call (_gate_pack), so that decode-only use never pays for it
            blk.mlp._w12g = None
            blk.mlp._w12g_f = None                            # ... and its norm-folded form (_folded), like the projections' below
            if isinstance(blk, _HyenaBlock):
                blk._wp_f = None
            else:
                blk.inner_mha_cls._wqkv_f = None
            blk.mlp._w12g_ok = (2 * ipad) % 256 == 0 and ipad % 32 == 0 and D_ % 64 == 0 and D_ >= 128
            if isinstance(blk, _HyenaBlock):
                f = blk.filter
                D = self.hidden_size
                f._fir_w = f.short_filter_weight.data.reshape(3 * D, self.short_filter_length).contiguous()
                f._poles = f.poles.data.reshape(D, self.state_size, 2).float().contiguous()
                f._residues = f.residues.data.reshape(D, self.state_size, 2).float().contiguous()
                # the [D,52,64] operand table of the matrix-core operator (54 MB per layer, 1.6 GB for the 29 Hyena layers of the 7B
                # model): built by _mfma_table on the first parallel Hyena call of the layer -- or up front by prepare() --, never for
                # decode-only use.  The operator reads the projection weight as it is (no regrouped copy).
                f._mfma_tab = None
                f._tab_prec = None                              # hyena_tables.table_precision's worst channel (decided with the table: _table_ok)
        self._packed = True

    def prepare(self, prefill: bool = True) -> "StripedHyena":
        """Builds the derived device-side tensors NOW instead of inside the first forward: the fused / padded MLP weights (always), and
        with `prefill` the regrouped l1 | l2 copies of the one-launch gated MLP (5.8 GB at 7B) and the Hyena layers' MFMA operand tables
        (1.6 GB) that prefill-sized batches use.  A server calls it at load time: an out-of-memory condition then surfaces before any
        KV cache or activation exists, the first request does not pay the packing, and the tensors are ordinary (not inference-mode)
        tensors whatever mode the first forward runs under.  Decode-only deployments pass prefill=False.
        Footprint at 7B: 12.9 GB of weights + 5.8 GB (l1 | l2 folded and regrouped) + 3.2 GB (folded projections / Wqkv) + 1.6 GB (operand
        tables).  A batch below 1,024 rows, a padding mask or `fuse_norm = False` later adds the UNFOLDED regrouped l1 | l2 (5.8 GB) on
        first use -- not covered by this call's out-of-memory check: `release_unused_weight_copies()` drops whichever set the current
        routing does not read, `fold_norms_()` keeps ONE weight set for good (14.5 GB)."""
        with torch.inference_mode(False), torch.no_grad():
            if not self._packed and not self._norms_folded:
                self._pack()
            if prefill:
                nf = self.ops.fuse_norm and self.blocks[0].mlp._w12g_ok
                for blk in self.blocks:
                    if self._norms_folded:
                        pass                                     # (one weight set: nothing to derive but the operand tables)
                    elif nf:                                   # the norm-folded copies the prefill launches read (see _nf_ok)
                        self._folded(blk.mlp, "_w12g_f", blk.mlp._w12, blk.post_norm.scale, gate=True)
                        if isinstance(blk, _HyenaBlock):
                            self._folded(blk, "_wp_f", blk.projections.weight, blk.pre_norm.scale)
                        else:
                            self._folded(blk.inner_mha_cls, "_wqkv_f", blk.inner_mha_cls.Wqkv.weight, blk.pre_norm.scale)
                    else:
                        self._gate_pack(blk, 1 << 20)
                    if isinstance(blk, _HyenaBlock) and self.ops.supports("hyena_ct") and self._table_ok(blk):
                        self._mfma_table(blk)
        return self

    # ------------------------------------------------------------------ one weight set (round 6)
    def fold_norms_(self) -> "StripedHyena":
        """ONE resident copy of every weight: the block norms' scale vectors are folded INTO the dense layers that consume them, in place --
        projections / Wqkv <- bf16(W diag(g_pre)), l1 | l2 <- bf16([W1; W2] diag(g_post)) kept only in the gated launch's row order, the
        scale vectors set to 1 -- and every derived copy is dropped (the unfolded regrouped l1 | l2, the folded projection copies).  The model
        is then the SAME function with unit norm scales (what the prefill path has computed since round 5: one rounding of the weight where
        the reference rounds the normalised activation); the decode launches take the same tensors (their RMSNorm multiplies by 1; the
        weight-streaming gate launches read l1 | l2 in the grouped order, include/evo_mi355x.h ABI 10).  Resident at 7B: 12.9 GB of weights +
        1.6 GB of Hyena operand tables instead of ~23.5 GB [REF evo/models.py:146-150: the reference holds one bf16 copy of the model].
        One-way: `state_dict()` afterwards returns the folded, unit-scale equivalent (l1 / l2 un-grouped on demand); moving the model to
        another device / dtype or loading another state dict needs a fresh model.  A serving deployment calls
        `model.to(device).prepare().fold_norms_()` once after loading."""
        if self._norms_folded:
            return self
        ops = self.ops
        with torch.inference_mode(False), torch.no_grad():
            if not self._packed:
                self._pack()
            for blk in self.blocks:
                mlp = blk.mlp
                inner = mlp.l1.weight.shape[0]
                w12f = Backend.fold_norm_scale(mlp._w12, blk.post_norm.scale.data)
                if mlp._w12g_ok and ops.supports("norm_fold"):     # (a backend with the folded launches reads l1 | l2 in the grouped order)
                    mlp._w12g = ops.pack_gate_weights(w12f)          # the ONLY copy of l1 | l2 from here on
                    mlp._w12 = None
                    mlp._l12_shape = (inner, w12f.shape[1])
                    mlp.l1.weight.data = w12f.new_empty(0)
                    mlp.l2.weight.data = w12f.new_empty(0)
                else:                                               # (toy dims outside the gated launch's contract: the plain order stays)
                    ipad = w12f.shape[0] // 2
                    mlp._w12 = w12f
                    mlp._w12g = None
                    mlp.l1.weight.data = w12f[:inner]
                    mlp.l2.weight.data = w12f[ipad:ipad + inner]
                mlp._w12g_f = None
                del w12f
                if isinstance(blk, _HyenaBlock):
                    blk.projections.weight.data = Backend.fold_norm_scale(blk.projections.weight.data, blk.pre_norm.scale.data)
                    blk._wp_f = None
                else:
                    mha = blk.inner_mha_cls
                    mha.Wqkv.weight.data = Backend.fold_norm_scale(mha.Wqkv.weight.data, blk.pre_norm.scale.data)
                    mha._wqkv_f = None
                blk.pre_norm.scale.data = torch.ones_like(blk.pre_norm.scale.data)
                blk.post_norm.scale.data = torch.ones_like(blk.post_norm.scale.data)
            self._norms_folded = True
            self._dgraph = None
            self._w8 = None                                   # (an FP8 set built before the fold holds the unfolded weights: rebuilt on next use)
        return self

    # ------------------------------------------------------------------ FP8 weights for the decode step
    def _w8_sources(self, blk) -> dict:
        """The dense weights a block's single-token step streams, as the bf16 decode launches read them."""
        mlp = blk.mlp
        if isinstance(blk, _HyenaBlock):
            w_in, w_out = blk.projections.weight.data, blk.out_filter_dense.weight.data
        else:
            w_in, w_out = blk.inner_mha_cls.Wqkv.weight.data, blk.inner_mha_cls.out_proj.weight.data
        # (l1 | l2: the padded plain order, or the grouped order after fold_norms_())
        return {"in": w_in, "out": w_out, "w12": mlp._w12 if mlp._w12 is not None else mlp._w12g, "w3": mlp._w3}

    def _padded_inner(self) -> int:
        """The MLP's inner size as _pack_impl pads it (the K of l3 and half the N of l1 | l2 that the decode launches see)."""
        inner = self.inner_size
        return ((inner + 255) // 256) * 256 if inner >= 1024 else inner

    def check_fp8_weights(self, rows: int = 1) -> None:
        """ValueError naming the first streamed layer the FP8 launches cannot take at `rows` batch rows -- K not a multiple of 16; above 8
        rows (the MFMA forms, csrc/skinny_fp8.hip) K not a multiple of 256; shapes only.  (The gate launch's I % 32 == 0 needs no line of
        its own: the inner size is l3's K.)"""
        D, ipad = self.hidden_size, self._padded_inner()
        for i, blk in enumerate(self.blocks):
            names = ("projections", "out_filter_dense") if isinstance(blk, _HyenaBlock) else ("inner_mha_cls.Wqkv", "inner_mha_cls.out_proj")
            for n, K in ((names[0], D), (names[1], D), ("mlp.l1 | mlp.l2", D), ("mlp.l3", ipad)):
                if K % 16:
                    raise ValueError(f'weight_dtype="fp8": blocks.{i}.{n} has K = {K}, not a multiple of 16 (include/evo_mi355x.h, ABI 20)')
                if rows > W8_MAX_ROWS and K % W8_WIDE_K:
                    raise ValueError(f'weight_dtype="fp8" at {rows} rows: blocks.{i}.{n} has K = {K}, not a multiple of {W8_WIDE_K} (the '
                                     f"launches for more than {W8_MAX_ROWS} rows; include/evo_mi355x.h, evo_linear_skinny_w8)")

    def prepare_fp8_weights(self) -> "StripedHyena":
        """Builds the FP8 (e4m3fn) copies of the dense weights a single-token step streams -- Hyena projections, Wqkv, out_filter_dense /
        out_proj, l1 | l2 (plain, or grouped after fold_norms_()) and l3, in whatever state the model is in -- NOW instead of inside the
        first `weight_dtype="fp8"` step: a server gets its out-of-memory error at load time.  The set sits BESIDE the bf16 weights, which
        prefill, scoring and embeddings keep reading: at 7B 6.45 GB + 4 bytes per output row more memory, for half the bytes per step.
        Embedding / unembedding, biases, norm scales, FIR taps, poles and residues stay as they are.  fold_norms_(), .to(...) and a new
        state dict drop the set (it is rebuilt on next use)."""
        ops = self.ops
        if not ops.supports("w_fp8"):
            raise RuntimeError('weight_dtype="fp8" needs a compute backend with the "w_fp8" kernels (' + ", ".join(Backend.OPTIONAL["w_fp8"])
                               + "); this model's backend has none")
        self.check_fp8_weights()
        if self._w8 is None:
            with torch.inference_mode(False), torch.no_grad():
                if not self._packed and not self._norms_folded:
                    self._pack()
                self._w8 = [{k: ops.w_quant_fp8(w) for k, w in self._w8_sources(blk).items()} for blk in self.blocks]
        return self

    def decode_weight_bytes(self, weight_dtype: str = "bf16") -> int:
        """Bytes of dense weights one single-token step streams in this format (the unembedding, bf16 in both, included); from shapes."""
        D, ipad = self.hidden_size, self._padded_inner()
        elems, rows = 4 * D * D + 3 * ipad * D, 5 * D + 2 * ipad          # per block: in [3D, D], out [D, D], l1 | l2 [2I, D], l3 [D, I]
        es = self.embedding_layer.weight.element_size()
        per_block = elems + 4 * rows if check_weight_dtype(weight_dtype) == "fp8" else elems * es
        return self.num_layers * per_block + (self.unembed.weight.numel() * es if self.has_own_unembed else 0)

    def release_unused_weight_copies(self) -> int:
        """Drops the derived weight copies the CURRENT routing does not read (a long-lived server that once ran a sub-1,024-row
        batch, a padding mask or `fuse_norm = False` holds the unfolded regrouped l1 | l2 (5.8 GB at 7B) beside the folded one that
        prepare() built; prepare()'s out-of-memory check covers only one of the two).  With the norms folded (the default) the unfolded
        regrouped copy goes, otherwise the folded ones; whatever is dropped is rebuilt on the next call that needs it.  Returns the bytes
        released.  (`fold_norms_()` is the permanent form: one weight set.)"""
        before = self.resident_bytes()
        fold = self.ops.fuse_norm
        for blk in ([] if self._norms_folded else self.blocks):
            if fold and blk.mlp._w12g_f is not None:
                blk.mlp._w12g = None
            if not fold:
                blk.mlp._w12g_f = None
                if isinstance(blk, _HyenaBlock):
                    blk._wp_f = None
                else:
                    blk.inner_mha_cls._wqkv_f = None
        return before - self.resident_bytes()

    def state_dict(self, *args, **kwargs):
        sd = super().state_dict(*args, **kwargs)
        if self._norms_folded:
            prefix = kwargs.get("prefix", args[1] if len(args) > 1 else "")
            for i, blk in enumerate(self.blocks):
                mlp = blk.mlp
                if mlp._w12 is None:                              # l1 / l2 live in the grouped buffer only: un-group on demand (a copy)
                    inner, K = mlp._l12_shape
                    g = mlp._w12g.view(-1, 2, 32, K)
                    sd[f"{prefix}blocks.{i}.mlp.l1.weight"] = g[:, 0].reshape(-1, K)[:inner]
                    sd[f"{prefix}blocks.{i}.mlp.l2.weight"] = g[:, 1].reshape(-1, K)[:inner]
        return sd

    def resident_bytes(self) -> int:
        """Device bytes this model holds: parameters, buffers and every derived tensor hanging off its modules (fused / regrouped / folded
        weight copies, Hyena operand tables), each storage counted once."""
        seen, total = set(), 0

        def add(t):
            nonlocal total
            if isinstance(t, torch.Tensor) and t.numel():
                st = t.untyped_storage()
                key = (st.data_ptr(), st.nbytes())
                if key not in seen:
                    seen.add(key)
                    total += st.nbytes()
        for mod in self.modules():
            for t in list(mod._parameters.values()) + list(mod._buffers.values()):
                add(t)
            for k, v in vars(mod).items():
                if k.startswith("_") and isinstance(v, torch.Tensor):
                    add(v)
        for rec in (r for layer in (self._w8 or []) for r in layer.values()):
            add(rec.data)
            add(rec.scale)
        return total

    # ------------------------------------------------------------------ caches
    def initialize_inference_params(self):
        """[REF evo/generation.py:116-120]"""
        return {
            "mha": InferenceParams(max_seqlen=self.max_seqlen, max_batch_size=1, seqlen_offset=0),
            "hyena": RecurrentInferenceParams(fir_filter_length=self.short_filter_length,
                                              state_dim=self.state_size, seqlen_offset=0),
        }

    def precompute_filters(self, L, device):
        """Upstream materialises h[D,L] here; this engine never builds the filter (it is evaluated through
        its modes on chip), so there is nothing to precompute.  Kept for API compatibility."""
        return None

    def _rotary(self, pos0: int, T: int, device) -> Tuple[torch.Tensor, torch.Tensor]:
        """cos/sin [T, hd/2] f32 for absolute positions pos0..pos0+T-1: fp32 angles (positions divided by
        the interpolation factor for the 131k model [REF evo-1-131k-base_inference.yml:39-40]) rounded to
        bf16 values, as flash-attn caches them in the activation dtype."""
        key = (pos0, T, str(device))
        hit = self._rot_cache.get(key)
        if hit is not None:
            return hit
        hit = self._rotary_dyn(torch.arange(pos0, pos0 + T, dtype=torch.float32, device=device))
        if len(self._rot_cache) > 8:               # a decode step reuses its table for all attention layers
            self._rot_cache.clear()
        self._rot_cache[key] = hit
        return hit

    def _row_index(self, B: int, device) -> torch.Tensor:
        hit = self._rows
        if hit is None or hit.numel() < B or hit.device != torch.device(device):
            hit = self._rows = torch.arange(max(B, 8), dtype=torch.int64, device=device)
        return hit[:B]

    def _inv_freq(self, dev) -> torch.Tensor:
        inv = self._inv_freq_dev
        if inv is None or inv.device != torch.device(dev):
            hd = self.head_dim
            inv = 1.0 / (self.rotary_base ** (torch.arange(0, hd, 2, dtype=torch.float32, device=dev) / hd))
            self._inv_freq_dev = inv
        return inv

    def _rotary_dyn(self, pos: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
        """The table for positions held in device memory ([n]; int64: one per decode stream) -- no host read, graph-capturable.
        Returns cos, sin [n, hd/2]."""
        inv = self._inv_freq(pos.device)
        t = pos.to(torch.float32)
        if self.rotary_scaling != 1.0:
            t = t / self.rotary_scaling
        freqs = torch.outer(t, inv)
        return (torch.cos(freqs).to(torch.bfloat16).float().contiguous(),
                torch.sin(freqs).to(torch.bfloat16).float().contiguous())

    # ------------------------------------------------------------------ blocks
    DECODE_ROWS = Backend.DECODE_ROWS         # batches this small take the fused single-token launches (Backend.fused_rows_ok)

    def _mixer_out_(self, blk, x2d, y, w, bias, mfma=False, w8=None, inv=False):
        """x += y @ w^T + bias, the mixer's output projection (bias in the dense layer's epilogue: one rounding where the reference rounds twice).
        `w8`: the block's FP8 weight records (a single-token step with weight_dtype == "fp8"), else None.  `inv`: a batch-invariant
        single-token step."""
        if inv:
            self.ops.linear_residual_rowinv_(x2d, y, w, bias=bias)
        elif w8 is not None:
            self.ops.linear_residual_w8_(x2d, y, w8["out"], bias=bias)
        elif y.dim() == 4:                                     # the Hyena operator's blocked output (ops.hyena_ct)
            self.ops.linear_residual_yblk_(x2d, y, w, bias=bias)
        else:
            self.ops.linear_residual_(x2d, y, w, mfma=mfma, bias=bias)

    def _finish_block(self, blk, x2d, y, w, bias, nf, mask=None, mfma=False, w8=None, inv=False):
        """Every block's end: x += y @ w^T + bias, then x += MLP(x).  `nf` (_nf_ok): returns the NEXT block's `rs`; else None.  `mask`: [B T, 1]."""
        if nf:
            return self._mlp_residual_rs_(blk, x2d, self._mixer_out_rs_(blk, x2d, y, w, bias))
        self._mixer_out_(blk, x2d, y, w, bias, mfma=mfma, w8=w8, inv=inv)
        self._mlp_residual_(blk, x2d, mask, w8=w8, inv=inv)
        return None

    # ---- RMSNorm folded into the dense layers around it (csrc/gemm.hip NF): `rs` = every row's 1 / (rms + eps), block to block
    def _nf_ok(self, M: int, mask) -> bool:
        ops, D = self.ops, self.hidden_size
        if mask is not None or not ops.fuse_norm or not ops.supports("norm_fold"):
            return False
        m0 = self.blocks[0].mlp
        ipad = (m0._w12 if m0._w12 is not None else m0._w12g).shape[0] // 2
        return (ops.nf_shape_ok(M, D, D) and ops.nf_shape_ok(M, 3 * D, D) and ops.nf_shape_ok(M, 2 * ipad, D) and ops.nf_shape_ok(M, D, ipad)
                and m0._w12g_ok and ops.mlp_gate_fused)

    def _folded(self, owner, name: str, w: torch.Tensor, g: torch.Tensor, gate: bool = False) -> torch.Tensor:
        """bf16(W diag(g)) of a norm-consuming layer (for l1 | l2: in the gated launch's row order), built on first use / by prepare()."""
        if self._norms_folded:                               # one weight set: the parameters ARE the folded weights (fold_norms_)
            return owner._w12g if gate else w.data
        hit = getattr(owner, name)
        if hit is None or hit.device != w.device:
            with torch.inference_mode(False), torch.no_grad():
                hit = self.ops.fold_norm_scale(w.data, g.data)
                if gate:
                    hit = self.ops.pack_gate_weights(hit)
            setattr(owner, name, hit)
        return hit

    def _mixer_out_rs_(self, blk, x2d, y, w, bias):
        """_mixer_out_ + the post-mixer norm's row factors."""
        if y.dim() == 4:
            return self.ops.linear_residual_yblk_stats_(x2d, y, w, bias, self.eps)
        return self.ops.linear_residual_stats_(x2d, y, w, bias, self.eps)

    def _mlp_residual_rs_(self, blk, x2d, rs_post):
        """The block's MLP on the raw stream (post-norm as a row factor in the gated launch), residual added in place; returns the NEXT
        pre-norm's row factors (l3's epilogue statistic)."""
        ops, mlp = self.ops, blk.mlp
        w12g_f = self._folded(mlp, "_w12g_f", mlp._w12, blk.post_norm.scale, gate=True)
        a = ops.mlp_gate_rs(x2d, rs_post, w12g_f, mlp._w12, blk.post_norm.scale, self.eps)
        return ops.linear_residual_stats_(x2d, a, mlp._w3, None, self.eps)

    def _gate_pack(self, blk, M: int):
        """The regrouped l1 | l2 weight of the one-launch gated MLP, built the first time a prefill-sized batch needs it."""
        mlp = blk.mlp
        if mlp._w12g is None and mlp._w12 is not None and M >= 256 and mlp._w12g_ok and self.ops.mlp_gate_fused:
            mlp._w12g = self.ops.pack_gate_weights(mlp._w12)
        return mlp._w12g

    def _mlp_residual_(self, blk, x2d, mask=None, w8=None, inv=False):
        """x += MLP(post_norm(x)), in place; `mask` (flat [B T, 1]): upstream's (mixer out + u) * padding_mask first."""
        ops = self.ops
        if inv:                                                          # norm, gate, l3: three launches at every row count
            n2 = ops.rmsnorm(x2d, None, blk.post_norm.scale, self.eps)
            ops.linear_residual_rowinv_(x2d, ops.mlp_gate_rowinv(n2, blk.mlp._w12, w12g=blk.mlp._w12g), blk.mlp._w3)
            return
        if w8 is not None:                                               # (single-token steps carry no mask)
            a = ops.mlp_gate_w8(x2d, w8["w12"], blk.post_norm.scale, self.eps, grouped=blk.mlp._w12 is None)
            ops.linear_residual_w8_(x2d, a, w8["w3"])
            return
        self._gate_pack(blk, x2d.shape[0])
        if mask is not None:
            x2d.mul_(mask)
            n2 = ops.rmsnorm(x2d, None, blk.post_norm.scale, self.eps)
            a = ops.mlp_gate(n2, blk.mlp._w12, w12g=blk.mlp._w12g)
        else:                                                            # norm + l1 / l2 + gate in one launch where the rows allow
            a = ops.mlp_gate(x2d, blk.mlp._w12, blk.post_norm.scale, self.eps, w12g=blk.mlp._w12g)
        ops.linear_residual_(x2d, a, blk.mlp._w3)

    def _mfma_hyena_ok(self, B: int, T: int) -> bool:
        """The single-pass matrix-core operator (csrc/hyena_ct.hip) serves every parallel (T > 1) Hyena call without a padding mask on
        the HIP backend -- scoring, cached prefill with carry-in / end state, sequence-parallel shards -- when the shape fits its launch
        contract; masks and very short inputs take the modal kernels.  (Shape part only: _hyena_ct_ok adds the tensors' checks.)"""
        return bool(T >= 32 and B * T >= 256 and self.hidden_size == self.num_heads * 128 and self.ops.hyena_mfma and self.ops.supports("hyena_ct"))

    def _mfma_table(self, blk):
        """The MFMA operand table of a Hyena block's filter (evo_amd/hyena_tables.py), built on first use."""
        f = blk.filter
        if f._mfma_tab is None or f._mfma_tab.device != blk.projections.weight.device:
            from ..hyena_tables import mfma_operand_table
            f._mfma_tab = mfma_operand_table(f._poles, f._residues, f.D.data)
        return f._mfma_tab

    def _table_ok(self, blk) -> bool:
        """Can this layer's filter go through the bf16 hi / lo operand tables of csrc/hyena_ct.hip?  (evo_amd/hyena_tables.py: filters whose
        modes cancel to ~1 % amplify the splits' 2^-16 to a bf16 rounding; such a layer runs the modal kernels -- fp32 states, every regime.)
        Decided once per layer from the poles / residues alone; `ops.hyena_table_guard = False` skips the check (tests of the guard itself)."""
        f = blk.filter
        if not self.ops.hyena_table_guard:
            return True
        from ..hyena_tables import TABLE_TOL, table_precision
        if f._tab_prec is None:
            f._tab_prec = float(table_precision(f._poles, f._residues, f.D.data).max())
        return f._tab_prec <= TABLE_TOL

    def _hyena_ct_ok(self, x2d, blk, B, T) -> bool:
        ops, w = self.ops, blk.projections.weight
        return (ops.hyena_ct_flag and ops.supports("hyena_ct") and x2d.is_cuda and w.dtype == torch.bfloat16
                and w.is_contiguous() and ops.zt_shape_ok(B, T, w.shape[0], w.shape[1]))

    def _hyena_block(self, i, blk, x2d, B, T, cache: Optional[RecurrentInferenceParams], mask=None, rs=None, w8=None, inv=False):
        """One Hyena block on the stream x2d [B T, D], in place; returns the next block's `rs` (or None).  Three routes: the decode step,
        the channel-major operator, the modal form.  `mask` = (flat [B*T,1] bf16, [B,T] uint8) of upstream's
        padding_mask, or None: the projections output, the FIR output and the mixer output + residual are multiplied by it, as upstream's
        ParallelGatedConvBlock / engine.parallel_fir do [UPSTREAM-RECALLED; evo never passes one, SURVEY 8b]."""
        have_state = cache is not None and i in cache.fir_state_dict
        lens = cache.lengths if cache is not None and T > 1 else None     # set by prefill_ragged: per-row end states
        if lens is not None and (have_state or mask is not None):
            raise ValueError("a ragged prefill (lengths) starts at t = 0 without a padding mask: no resumed prefill, no mask")
        nf = False
        w8 = w8 if have_state and T == 1 else None            # (only the single-token cached route takes the FP8 launches)
        inv = inv and have_state and T == 1                   # (and only it the row-invariant ones)
        if inv:                                               # norm, projection, step: the unfused sequence, at every row count
            f = blk.filter
            z = self.ops.linear_rowinv(self.ops.rmsnorm(x2d, None, blk.pre_norm.scale, self.eps), blk.projections.weight, blk.projections.bias)
            y = self.ops.hyena_step(z, cache.fir_state_dict[i], cache.state_dict[i], f._fir_w, f.short_filter_bias, f._poles, f._residues, f.D,
                                    self.num_heads)
        elif have_state and T == 1:
            y = self._hyena_decode_step(blk, x2d, cache.fir_state_dict[i], cache.state_dict[i], w8)
        elif mask is None and self._mfma_hyena_ok(B, T) and self._hyena_ct_ok(x2d, blk, B, T) and self._table_ok(blk):
            nf = self._nf_ok(B * T, mask)
            y = self._hyena_channel_major(i, blk, x2d, B, T, cache, lens, rs, nf)
        else:
            y = self._hyena_modal(i, blk, x2d, B, T, cache, lens, mask)
        return self._finish_block(blk, x2d, y, blk.out_filter_dense.weight, blk.out_filter_dense.bias, nf, None if mask is None else mask[0], w8=w8,
                                  inv=inv)

    def _hyena_decode_step(self, blk, x, fir_state, iir_state, w8=None):
        """One token per row: norm + projections + FIR / modal step + gate in one launch; the two states advance in place.  `w8`: the
        block's FP8 weight records, or None (bf16: the scoring path's tail split always)."""
        f = blk.filter
        if w8 is not None:
            return self.ops.hyena_decode_fused_w8(x, blk.pre_norm.scale, self.eps, w8["in"], blk.projections.bias, fir_state, iir_state,
                                                  f._fir_w, f.short_filter_bias, f._poles, f._residues, f.D, self.num_heads)
        return self.ops.hyena_decode_fused(x, blk.pre_norm.scale, self.eps, blk.projections.weight, blk.projections.bias, fir_state, iir_state,
                                           f._fir_w, f.short_filter_bias, f._poles, f._residues, f.D, self.num_heads)

    @staticmethod
    def _carry_in(cache, i):
        """(halo [B, 2, 3 D], s0) of the cached prefix layer i continues with more than one token, (None, None) at t = 0."""
        if cache is None or i not in cache.fir_state_dict:
            return None, None
        return cache.fir_state_dict[i].transpose(1, 2).contiguous(), cache.state_dict[i]

    def _hyena_z(self, blk, x2d, rs, B, T, tail=True, zt=True, nf=False):
        """How a Hyena block's projection z comes about -> (normed, project).  The pre-norm pass, if the form has one, is launched HERE;
        `project()` -- to be called exactly ONCE -- launches the projection and returns z: sp.py puts its halo rows' launches in between.
          1. zt, nf, rs given, zt_stream_rows_ok: the swapped-operand dense layer reads the stream itself, rs in its epilogue  -> z^T
          2. zt: the pre-norm writes its rows in z^T's position order (rmsnorm_rows), then the swapped-operand layer          -> z^T
          3. otherwise: norm, then the plain dense layer -> token-major z [B, T, 3 D]; `normed` = the normalised rows (else None)
        z^T: channel-major [blocks, 3 D, 256] (Backend.zt_layout; `tail=False` leaves its tail block out); the weight is read as it is."""
        ops = self.ops
        w, scale = blk.projections.weight.data, blk.pre_norm.scale
        pb = None if blk.projections.bias is None else blk.projections.bias.data
        if zt and nf and rs is not None and ops.zt_stream_rows_ok(B, T):
            return None, lambda: ops.linear_t_rs(x2d, rs, self._folded(blk, "_wp_f", blk.projections.weight, scale), pb, w, scale, self.eps,
                                                 B, T, tail=tail)
        if zt:
            xp = ops.rmsnorm_rows(x2d, scale, self.eps, B, T)
            return None, lambda: ops.linear_t(xp, w, pb, B, T, tail=tail)
        n1 = ops.rmsnorm(x2d, None, scale, self.eps)
        return n1, lambda: ops.linear(n1, w, pb).view(B, T, w.shape[0])

    def _hyena_channel_major(self, i, blk, x2d, B, T, cache, lens, rs, nf):
        """The whole operator in ONE pass on the matrix cores (csrc/hyena_ct.hip) -- scoring and cached prefill (carry-in state + FIR
        history in, end state out) alike -- on z^T (_hyena_z: a lane's eight steps of a channel are 16 contiguous bytes, no window in LDS).
        Returns y BLOCKED: the operator stores whole cache lines and the output projection gathers them -- no row-major y on this route."""
        ops = self.ops
        D, H, f = self.hidden_size, self.num_heads, blk.filter
        K1 = self.short_filter_length - 1
        table = self._mfma_table(blk)
        # tail split (T = 512 k + 1 scoring, ops.hyena_tail_split): the one token behind every row's whole tiles takes the fused single-token
        # launch from the operator's end state, not a ragged tile (HipOps.hyena_ct, main_only)
        Tm, _, _, r_tail = ops.zt_layout(B, T)
        split = (cache is None and r_tail == 1 and ops.hyena_tail_split and Backend.fused_rows_ok(B, D) and blk.projections.bias is not None)
        zt = self._hyena_z(blk, x2d, rs, B, T, tail=not split, nf=nf)[1]()
        yb = ops.yblk_empty(B * T, D, zt.device)
        if split:
            _, state = ops.hyena_ct(zt, B, T, f._fir_w, f.short_filter_bias, table, H, want_state=True, poles=f._poles, y_blk=yb, main_only=True)
            ix = self._tail_split_index(B, T, zt.device)
            fir = zt[ix["zblk"], :, 256 - K1:].contiguous()                         # [B, 3 D, 2]: steps Tm - 2, Tm - 1 of every row, oldest first
            x_tail = x2d.view(B, T, D)[:, Tm].contiguous()                          # the raw stream's rows (the launch norms them itself)
            yb[ix["yblk"], :, ix["yrow"], :] = self._hyena_decode_step(blk, x_tail, fir, state).view(B, D // 16, 16)   # rows b T + Tm of the blocked y
        elif cache is None or lens is not None:
            ops.hyena_ct(zt, B, T, f._fir_w, f.short_filter_bias, table, H, y_blk=yb)
            if lens is not None:             # ragged batch: state and FIR history at every row's OWN last token (csrc/hyena_ragged.hip)
                cache.state_dict[i], cache.fir_state_dict[i] = ops.hyena_state_at_zt(zt, B, T, lens, f._fir_w, f.short_filter_bias, f._poles, H)
        else:
            halo, s0 = self._carry_in(cache, i)
            _, cache.state_dict[i] = ops.hyena_ct(zt, B, T, f._fir_w, f.short_filter_bias, table, H, z_halo=halo, s0=s0, want_state=True,
                                                  poles=f._poles, y_blk=yb)
            cache.fir_state_dict[i] = ops.zt_rows(zt, B, T, T - K1, K1).transpose(1, 2).contiguous()   # [B, 3D, 2]
        return yb

    def _hyena_modal(self, i, blk, x2d, B, T, cache, lens, mask):
        """The three-launch modal form on token-major z (fp32 states, every regime).  Returns y [B T, D]."""
        ops = self.ops
        D, H, f = self.hidden_size, self.num_heads, blk.filter
        K1 = self.short_filter_length - 1
        z = ops.norm_linear(x2d, blk.pre_norm.scale, self.eps, blk.projections.weight, blk.projections.bias)   # [B*T, 3D]
        if mask is not None:
            z.mul_(mask[0])
        z3 = z.view(B, T, 3 * D)
        halo, s0 = self._carry_in(cache, i)
        y3, state = ops.hyena_prefill(z3, f._fir_w, f.short_filter_bias, f._poles, f._residues, f.D, H, z_halo=halo, s0=s0,
                                      want_state=cache is not None and lens is None, mask=None if mask is None else mask[1])
        if lens is not None:
            cache.state_dict[i], cache.fir_state_dict[i] = ops.hyena_state_at(z3, lens, f._fir_w, f.short_filter_bias, f._poles, H)
        elif cache is not None:
            tail = z3[:, -K1:, :]
            if T < K1:                           # (a one-token prefill of a fresh cache; with state, one token is the decode step)
                tail = torch.cat([z3.new_zeros(B, K1 - T, 3 * D), tail], dim=1)
            cache.fir_state_dict[i] = tail.transpose(1, 2).contiguous()      # [B, 3D, 2]
            cache.state_dict[i] = state
        return y3.view(B * T, D)

    def _tail_split_index(self, B: int, T: int, device):
        """Index tensors of the tail-split routing (_hyena_block), cached per (B, T): the z^T block holding the last two main steps of every
        batch row, and block / row of the blocked y for the rows b T + Tm."""
        key = (B, T, str(device))
        cur = self._tail_ix
        if cur is None or cur[0] != key:
            Tm = self.ops.zt_layout(B, T)[0]
            b = torch.arange(B, device=device)
            R = b * T + Tm
            cur = (key, {"zblk": (b * Tm + Tm - 1) // 256, "yblk": R // self.ops.YBLK, "yrow": R % self.ops.YBLK})
            self._tail_ix = cur
        return cur[1]

    def _kv_buffer(self, cache: InferenceParams, i: int, B: int, need: int, like):
        """Layer i's KV buffer with room for B rows of `need` tokens on `like`'s device: a bf16 tensor, or with cache.kv_dtype == "fp8" an
        Fp8KV record (both of its tensors are allocated, grown and copied together)."""
        H, hd = self.num_heads, self.head_dim
        kv = cache.key_value_memory_dict.get(i)
        if isinstance(kv, PagedKV) or cache.kv_layout != "contiguous":
            raise ValueError(f"layer {i}: a paged KV cache is sized by its pool and never grown or allocated here (kv_layout = "
                             f"{cache.kv_layout!r}; it serves the decode pool's per-row single-token step only)")
        fp8 = cache.kv_dtype == "fp8"
        if kv is not None and isinstance(kv, Fp8KV) != fp8:
            raise ValueError(f"layer {i}'s KV cache does not have the format kv_dtype = {cache.kv_dtype!r} names")
        cap_b = max(int(cache.max_batch_size or 1), B)
        if kv is None or kv.shape[0] < B or kv.shape[1] < need or kv.device != like.device:
            cap_t = max(int(cache.max_seqlen or 0), need)
            if kv is not None and kv.shape[1] < need:
                cap_t = max(cap_t, 2 * kv.shape[1])           # grow geometrically past max_seqlen (a20)
            if fp8:
                new = Fp8KV.zeros(cap_b, cap_t, H, hd, like.device)
                if kv is not None:
                    b0, t0 = min(kv.shape[0], cap_b), min(kv.shape[1], cap_t)
                    new.data[:b0, :t0] = kv.data[:b0, :t0].to(like.device)
                    new.scale[:b0, :, :, :t0] = kv.scale[:b0, :, :, :t0].to(like.device)
            else:
                new = torch.zeros(cap_b, cap_t, 2, H, hd, dtype=like.dtype, device=like.device)
                if kv is not None:
                    b0, t0 = min(kv.shape[0], cap_b), min(kv.shape[1], cap_t)
                    new[:b0, :t0] = kv[:b0, :t0].to(like.device)
            cache.key_value_memory_dict[i] = kv = new
        return kv

    def _attn_block(self, i, blk, x2d, B, T, cache: Optional[InferenceParams], mask=None, rs=None, w8=None, inv=False):
        """One attention block on the stream x2d [B T, D], in place; returns the next block's `rs` (or None).  After Wqkv, by the cache:
        per-row decode step (pos_tensor), shared-prefix attention, scalar-offset decode step, causal attention; an FP8
        cache (cache.kv_dtype == "fp8") takes _attn_fp8 for all of them."""
        ops = self.ops
        D, H, hd = self.hidden_size, self.num_heads, self.head_dim
        mha = blk.inner_mha_cls
        if mask is not None:                      # upstream AttentionBlock: u * padding_mask before and after the mixer
            x2d.mul_(mask[0])
        nf = T > 1 and self._nf_ok(B * T, mask)
        # (only the decode branch -- one token on a layer that holds keys -- takes the FP8 launches)
        w8 = w8 if T == 1 and cache is not None and i in cache.key_value_memory_dict else None
        # a batch-invariant step: the per-row decode branch on a bf16 cache, contiguous or paged, with a fixed split count
        inv = inv and T == 1 and cache is not None and i in cache.key_value_memory_dict
        if inv and (cache.pos_tensor is None or cache.pos_tensor.numel() != B or cache.prompt_store is not None or cache.kv_dtype != "bf16"):
            raise ValueError("a batch-invariant step is the per-row single-token step (pos_tensor, one position per row) on a bf16 KV cache "
                             "without a prompt store")
        splits = ROWINV_SPLITS if inv else None
        if inv:
            qkv = ops.linear_rowinv(ops.rmsnorm(x2d, None, blk.pre_norm.scale, self.eps), mha.Wqkv.weight, mha.Wqkv.bias).view(B, T, 3, H, hd)
        elif w8 is not None:
            qkv = ops.norm_linear_w8(x2d, blk.pre_norm.scale, self.eps, w8["in"], mha.Wqkv.bias).view(B, T, 3, H, hd)
        elif nf and rs is not None:
            wqkv_f = self._folded(mha, "_wqkv_f", mha.Wqkv.weight, blk.pre_norm.scale)
            qkv = ops.linear_rs(x2d, rs, wqkv_f, mha.Wqkv.bias, mha.Wqkv.weight, blk.pre_norm.scale, self.eps).view(B, T, 3, H, hd)
        else:
            qkv = ops.norm_linear(x2d, blk.pre_norm.scale, self.eps, mha.Wqkv.weight, mha.Wqkv.bias, mfma=True).view(B, T, 3, H, hd)
        off = int(cache.seqlen_offset) if cache is not None else 0
        pos = cache.pos_tensor if cache is not None else None
        shared = cache.shared_prefix if cache is not None else None
        if T > 1 and cache is not None and cache.lengths is not None and (off != 0 or mask is not None or shared is not None):
            raise ValueError("a ragged prefill (lengths) starts at t = 0 with keys of its own: no resumed prefill, no mask, no shared_prefix")
        q = qkv[:, :, 0]
        # ops.attn_prescale: the rotary kernel folds softmax_scale * log2(e) into its one rounding of q, the attention kernels take scores as exponents
        pre = bool(ops.attn_prescale)
        q_scale = ops.attn_q_scale(hd) if pre else 1.0
        if cache is not None and (cache.kv_layout != "contiguous" or isinstance(cache.key_value_memory_dict.get(i), PagedKV)):
            a = self._attn_paged(i, qkv, B, T, cache, off, pos, mask, pre, q_scale, splits)
        elif cache is not None and cache.kv_dtype != "bf16":
            a = self._attn_fp8(i, qkv, B, T, cache, off, pos, mask, pre, q_scale)
        elif pos is not None and T == 1:
            # one position PER ROW, in device memory (hipGraph replay, continuous batching); behind a prompt store the append goes to the row's OWN index
            kv = cache.key_value_memory_dict[i][:B]
            store = cache.prompt_store
            widx = store.own_pos if store is not None else None
            if ops.supports("rope_append_decode") and pos.numel() == B:
                # rotary at each row's position + the KV append in one launch (no per-step cos / sin table)
                ops.rope_append_decode(qkv, kv, pos, self._inv_freq(x2d.device), self.rotary_scaling, q_scale=q_scale, widx=widx)
            else:
                # the rotary kernel indexes its table by token, so the B rows are presented as one sequence of B tokens with the per-row table
                cos, sin = cache._rot_dyn or self._rotary_dyn(pos)
                ops.rope_(qkv.view(1, B, 3, H, hd), cos, sin, q_scale=q_scale)
                kv[self._row_index(B, x2d.device), pos if widx is None else widx] = qkv[:, 0, 1:3]
            if store is not None:
                skv = store.kv[i]
                a = ops.attention_decode_prefix(q, kv[:, :, 0], kv[:, :, 1], widx, skv[:, :, 0], skv[:, :, 1], store.row, store.length,
                                                prescaled=pre)
            else:
                a = ops.attention_decode(q, kv[:, :, 0], kv[:, :, 1], pos=pos, n_splits=splits, prescaled=pre)
        else:
            cos, sin = self._rotary(off, T, x2d.device)
            ops.rope_(qkv, cos, sin, q_scale=q_scale)
            if shared is not None:
                # every row continues the first `off` tokens of ONE reference (score_variants), read from its own buffer: no per-row KV buffer
                kvr = shared.kv[i]
                a = ops.attention_prefix(q, qkv[:, :, 1], qkv[:, :, 2], kvr[0, :off, 0], kvr[0, :off, 1], vt_pre=shared.vt.get(i), prescaled=pre)
            else:
                if cache is not None:
                    kv = self._kv_buffer(cache, i, B, off + T, qkv)
                    kv[:B, off:off + T].copy_(qkv[:, :, 1:3])
                    k, v = kv[:B, : off + T, 0], kv[:B, : off + T, 1]
                else:
                    k, v = qkv[:, :, 1], qkv[:, :, 2]
                if T == 1 and cache is not None:
                    a = ops.attention_decode(q, k, v, prescaled=pre)      # split-K over the KV cache
                else:
                    a = ops.attention(q, k, v, off, prescaled=pre)
        return self._finish_block(blk, x2d, a.view(B * T, D), mha.out_proj.weight, mha.out_proj.bias, nf, None if mask is None else mask[0],
                                  mfma=True, w8=w8, inv=inv)

    def _attn_fp8(self, i, qkv, B, T, cache: InferenceParams, off: int, pos, mask, pre: bool, q_scale: float):
        """_attn_block's attention on an FP8 KV cache (cache.kv_dtype == "fp8"): a fresh prefill attends to its own bf16
        q / k / v exactly as with a bf16 cache -- only the store is quantised -- and a single-token step reads the FP8 cache."""
        ops = self.ops
        check_kv_dtype(cache.kv_dtype)
        if not ops.supports("kv_fp8"):
            raise RuntimeError('kv_dtype="fp8" needs a compute backend with the "kv_fp8" kernels (kv_quant_fp8, rope_append_decode_fp8, '
                               "attention_decode_fp8); this model's backend has none")
        for what, bad in (("shared_prefix", cache.shared_prefix is not None), ("prompt_store", cache.prompt_store is not None),
                          ("a padding mask", mask is not None),
                          (f"a resumed multi-token prefill (T = {T} at offset {off})", T > 1 and (off > 0 or pos is not None))):
            if bad:
                raise ValueError(f'kv_dtype="fp8" does not combine with {what}: the FP8 cache serves a fresh prefill and single-token steps')
        q = qkv[:, :, 0]
        if pos is not None:                                   # one position per row, in device memory (the pool, the captured step)
            if pos.numel() != B:
                raise ValueError(f'kv_dtype="fp8": pos_tensor must hold one position per row ({B}), got {pos.numel()}')
            kv = cache.key_value_memory_dict[i].rows(B)
            ops.rope_append_decode_fp8(qkv, kv, pos, self._inv_freq(qkv.device), self.rotary_scaling, q_scale=q_scale)
            return ops.attention_decode_fp8(q, kv, pos=pos, prescaled=pre)
        cos, sin = self._rotary(off, T, qkv.device)
        ops.rope_(qkv, cos, sin, q_scale=q_scale)
        kv = self._kv_buffer(cache, i, B, off + T, qkv).rows(B)
        ops.kv_quant_fp8(qkv[:, :, 1], qkv[:, :, 2], kv, t0=off)
        if off > 0:                                           # (T == 1) a single-token step at a scalar offset (Generator)
            return ops.attention_decode_fp8(q, kv, n_keys=off + 1, prescaled=pre)
        # a fresh prefill, one-token prompts included: its own keys, through the launch a bf16 cache would take
        if T == 1:
            return ops.attention_decode(q, qkv[:, :, 1], qkv[:, :, 2], prescaled=pre)
        return ops.attention(q, qkv[:, :, 1], qkv[:, :, 2], 0, prescaled=pre)

    def _attn_paged(self, i, qkv, B, T, cache: InferenceParams, off: int, pos, mask, pre: bool, q_scale: float, n_splits=None):
        """_attn_block's attention on a paged KV cache (cache.kv_layout == "paged"): the per-row single-token step of a
        decode pool and nothing else -- prompts are prefilled on contiguous caches of their own and copied into pages."""
        ops = self.ops
        kv = cache.key_value_memory_dict.get(i)
        if cache.kv_layout != "paged" or not isinstance(kv, PagedKV):
            raise ValueError(f"layer {i}'s KV cache does not have the layout kv_layout = {cache.kv_layout!r} names")
        for what, bad in (("shared_prefix", cache.shared_prefix is not None), ("prompt_store", cache.prompt_store is not None),
                          ('kv_dtype="fp8"', cache.kv_dtype != "bf16"), ("a padding mask", mask is not None),
                          (f"a multi-token forward (T = {T})", T > 1),
                          ("a scalar-offset step (no pos_tensor)", T == 1 and pos is None)):
            if bad:
                raise ValueError(f'kv_layout="paged" does not combine with {what}: the paged cache serves per-row single-token steps')
        if pos.numel() != B:
            raise ValueError(f'kv_layout="paged": pos_tensor must hold one position per row ({B}), got {pos.numel()}')
        if not ops.supports("kv_paged"):
            raise RuntimeError('kv_layout="paged" needs a compute backend with the "kv_paged" kernels (rope_append_decode_paged, '
                               "attention_decode_paged); this model's backend has none")
        kv = kv.rows(B)
        ops.rope_append_decode_paged(qkv, kv, pos, self._inv_freq(qkv.device), self.rotary_scaling, q_scale=q_scale)
        return ops.attention_decode_paged(qkv[:, :, 0], kv, pos, n_splits=n_splits, prescaled=pre)

    # ------------------------------------------------------------------ forward
    max_rows_per_pass = 160 * 1024     # rows (B T) of one stateless pass; larger batches run in row groups (hidden_states)

    def _row_groups(self, B: int, T: int):
        """How a stateless pass over B rows of T tokens is run: [B] (one pass) or the sizes of the row groups run one after the other.
        Batch rows are independent and every launch is row-independent, so grouping changes no row's arithmetic except through which
        rows fall beyond a multiple of 256 (they take the weight-streaming launches).  Two reasons to group:
        (1) more rows than `max_rows_per_pass`: the persistent dense layers address their operands with 32-bit offsets (4 GiB: z^T at
            174 k positions, l3's input at 195 k rows); beyond that a pass would leave them for the library / three-launch routing --
            e.g. scripts/score.py's default batch of 32 sequences at 8 k nt;
        (2) a pass of >= 64 k rows whose rows beyond a multiple of 256 do not fit the fused single-token launches (> 8 rows, e.g.
            16 x 8,193): its norms and gates would run unfused.
        Groups are balanced, as few as fit, and preferably with <= 8 such rows each, as long as every group keeps >= 32 k rows (enough
        tiles for 256 CUs; the per-group launch overhead is ~1e-4 of its time)."""
        cap = max(1, self.max_rows_per_pass // T)

        def fits(p):
            r = (p * T) % 256                                # (grouping is decided for the 7B width, where up to DECODE_ROWS rows fit)
            return r == 0 or Backend.fused_rows_ok(r, 4096)

        if B <= cap and (fits(B) or B * T < 65536):
            return [B]
        n0 = (B + cap - 1) // cap

        def split(n):
            q, r = divmod(B, n)
            return [q + 1] * r + [q] * (n - r)

        n = n0
        while n <= B and (B // n) * T >= 32768:
            g = split(n)
            if all(fits(p) for p in set(g)):
                return g
            n += 1
        return split(n0)

    def hidden_states(self, x: torch.Tensor, inference_params_dict=None, padding_mask=None) -> torch.Tensor:
        """ids [B,T] -> final-norm hidden states [B*T, D] (logits = hidden @ E^T)."""
        if not self._packed:
            self._pack()
        if x.dim() != 2:
            raise ValueError("input_ids must be [batch, length]")
        B, T = x.shape
        ops = self.ops
        if padding_mask is not None and tuple(padding_mask.shape) != (B, T):
            raise ValueError(f"padding_mask must be [batch, length] = {(B, T)}, got {tuple(padding_mask.shape)}")
        groups = self._row_groups(B, T) if inference_params_dict is None else [B]
        if len(groups) > 1:
            out, b0 = None, 0
            for nb in groups:
                pm = None if padding_mask is None else padding_mask[b0:b0 + nb]
                hg = self.hidden_states(x[b0:b0 + nb], None, pm)
                if out is None:
                    out = torch.empty(B * T, hg.shape[1], dtype=hg.dtype, device=hg.device)
                out[b0 * T:(b0 + nb) * T] = hg
                b0 += nb
            return out
        h = ops.embed(x.to(self.device), self.embedding_layer.weight)             # [B*T, D]
        mask = None
        if padding_mask is not None:
            pm = padding_mask.to(self.device) != 0
            mask = (pm.reshape(B * T, 1).to(h.dtype), pm.to(torch.uint8).contiguous())
        mha_c, hy_c = (inference_params_dict["mha"], inference_params_dict["hyena"]) if inference_params_dict is not None else (None, None)
        dyn = T == 1 and mha_c is not None and mha_c.pos_tensor is not None
        if dyn and not ops.supports("rope_append_decode"):   # (fallback path) one rotary table per decode step for all layers
            mha_c._rot_dyn = self._rotary_dyn(mha_c.pos_tensor)
        try:
            self._run_blocks(h, B, T, mha_c, hy_c, mask)
        finally:
            if dyn:
                mha_c._rot_dyn = None
        if self.norm is not None:
            h = ops.rmsnorm(h, None, self.norm.scale, self.eps)
        return h

    def _run_blocks(self, h: torch.Tensor, B: int, T: int, mha_c, hy_c, mask, stop: Optional[int] = None, after_block=None) -> None:
        """Blocks 0 .. stop - 1 (default: all) on the residual stream h [B T, D], in place.  `after_block(i, h)` is called as soon as
        block i has finished (StripedHyena.embeddings pools the streams it asked for there)."""
        stop = self.num_layers if stop is None else stop
        rs = None
        w8s = None
        if T == 1 and mha_c is not None and check_weight_dtype(mha_c.weight_dtype) == "fp8":     # 
            check_weight_rows(B, "batch rows", self.ops.W8_ROWS)
            if B > W8_MAX_ROWS:
                self.check_fp8_weights(B)
            w8s = self.prepare_fp8_weights()._w8
        inv = T == 1 and mha_c is not None and bool(mha_c.batch_invariant)                         # 
        if inv:
            if w8s is not None:
                raise ValueError('batch_invariant does not combine with weight_dtype="fp8": the row-invariant launches are bf16')
            check_rowinv_rows(B, "batch rows")
            if not self.ops.supports("row_invariant", "hyena_step"):
                raise RuntimeError('batch_invariant needs a compute backend with the "row_invariant" kernels ('
                                   + ", ".join(Backend.OPTIONAL["row_invariant"]) + ") and hyena_step; this model's backend has none")
        taps, tap_idxs = self.block_taps, self.block_tap_idxs
        for i in range(stop):
            blk = self.blocks[i]
            if taps is not None and (tap_idxs is None or i in tap_idxs):
                taps.append(h.clone())
            # rs: 1 / (rms + eps) of every row of h, from the epilogue of the dense layer that wrote it (None: the block norms h itself)
            if isinstance(blk, _AttentionBlock):
                rs = self._attn_block(i, blk, h, B, T, mha_c, mask, rs, w8=None if w8s is None else w8s[i], inv=inv)
            else:
                rs = self._hyena_block(i, blk, h, B, T, hy_c, mask, rs, w8=None if w8s is None else w8s[i], inv=inv)
            if after_block is not None:
                after_block(i, h)
        if stop == self.num_layers and taps is not None and (tap_idxs is None or self.num_layers in tap_idxs):
            taps.append(h.clone())

    @torch.no_grad()
    def embeddings(self, input_ids: torch.Tensor, layers, pooling: str = "mean", start: int = 1, lengths=None,
                   padding_mask=None, inference_params_dict=None) -> Dict:
        """Sequence embeddings of ids [B, T] in ONE partial forward: {layer: tensor} for every requested layer.

        layers:  block indices k in [0, num_layers) -- the residual stream LEAVING block k (what block_taps records as the input of
                 block k + 1) -- and / or "final", the final-norm output (hidden_states()' result).  The blocks run up to the deepest
                 one requested and stop there; the unembedding never runs.
        pooling: "mean" / "last" over positions [start, start + lengths[b]) of row b (default start = 1: the BOS of prepare_batch is
                 skipped; lengths default to T - start; pads beyond a row's length are never pooled) -> [B, D] fp32, pooled by the
                 pooling kernel (csrc/pool.hip) as soon as the layer's block finishes; for "final" with the RMSNorm fused in (the normed
                 [B T, D] is never written).  "none": the per-position rows, [B, T, D] bf16 (for "final" bit for bit hidden_states()).
        Batches beyond max_rows_per_pass run in row groups (_row_groups), as hidden_states does.  Not supported: a padding mask, an
        inference cache, a model whose weights are not on the GPU."""
        from ..embeddings import check_pooling, normalize_layers
        if padding_mask is not None:
            raise ValueError("embeddings: padding_mask is not supported (pass the true lengths instead: pads are never pooled)")
        if inference_params_dict is not None:
            raise ValueError("embeddings: an inference cache is not supported (embeddings are a stateless forward)")
        if not self.embedding_layer.weight.is_cuda:
            raise RuntimeError(f"embeddings: the model's weights are on {self.embedding_layer.weight.device}; move the model to the GPU")
        layers = normalize_layers(layers, self.num_layers)
        check_pooling(pooling)
        if input_ids.dim() != 2:
            raise ValueError("input_ids must be [batch, length]")
        B, T = input_ids.shape
        if lengths is None:
            lengths = [T - start] * B
        lengths = [int(n) for n in lengths]
        if len(lengths) != B:
            raise ValueError(f"embeddings: {len(lengths)} lengths for a batch of {B}")
        if start < 0 or any(n < 1 or start + n > T for n in lengths):
            raise ValueError(f"embeddings: every row needs 1 <= length and start + length <= T = {T} (start {start}, lengths {lengths})")
        if not self._packed:
            self._pack()
        ops = self.ops
        D = self.hidden_size
        dev = self.device
        blocks = [l for l in layers if l != "final"]
        stop = self.num_layers if "final" in layers else max(blocks) + 1
        out = {l: (torch.empty(B, T, D, dtype=torch.bfloat16, device=dev) if pooling == "none"
                   else torch.empty(B, D, dtype=torch.float32, device=dev)) for l in layers}
        b0 = 0
        for nb in self._row_groups(B, T):
            ranges = [(b * T + start, lengths[b0 + b]) for b in range(nb)]

            def take(l, hh, scale=None, b0=b0, nb=nb, ranges=ranges):
                if pooling == "none":
                    out[l][b0:b0 + nb] = hh.view(nb, T, D)
                else:
                    out[l][b0:b0 + nb] = ops.pool_rows(hh, ranges, scale=scale, eps=self.eps, mode=pooling)

            def after_block(i, hh):
                if i in blocks:
                    take(i, hh)

            h = ops.embed(input_ids[b0:b0 + nb].to(dev), self.embedding_layer.weight)
            self._run_blocks(h, nb, T, None, None, None, stop=stop, after_block=after_block)
            if "final" in layers:
                if self.norm is None:
                    take("final", h)
                elif pooling == "none":
                    take("final", ops.rmsnorm(h, None, self.norm.scale, self.eps))
                else:
                    take("final", h, scale=self.norm.scale)
            b0 += nb
        return out

    @torch.no_grad()
    def forward(self, x, inference_params_dict=None, padding_mask=None):
        """(logits [B,T,V] bf16, cache-or-None).  `padding_mask` [B,T] (1 = token, 0 = pad) is applied as upstream's
        stateless_forward applies it (block inputs / FIR output / mixer output multiplied by it); evo itself never passes
        one [REF evo/scoring.py:81; evo/generation.py:152-155] -- without it pads are ordinary tokens.  It is a scoring
        option: with a cache the call is upstream's stateful_forward, which ignores the mask -- so does this (with a warning)."""
        B, T = x.shape
        if padding_mask is not None and inference_params_dict is not None:
            # upstream routes this call to stateful_forward, which never looks at the mask: same here (a caller written against
            # upstream keeps working); the warning says that pads then enter the carried modal / FIR / KV state as ordinary tokens
            import warnings
            warnings.warn("padding_mask is ignored when inference_params_dict is given (as in upstream's stateful_forward)")
            padding_mask = None
        if T == 1 and inference_params_dict is not None and self._graph_eligible(inference_params_dict):     # (a cache: no mask, above)
            logits = self._graph_decode_step(x, inference_params_dict)
            if logits is not None:
                return logits, inference_params_dict
        h = self.hidden_states(x, inference_params_dict, padding_mask)
        return self._unembed_output(h, B, T), inference_params_dict

    @torch.no_grad()
    def prefill_ragged(self, ids: torch.Tensor, lengths, pad_to: int = 64, inference_params_dict=None, padding_mask=None,
                       kv_dtype: str = "bf16"):
        """Cached prefill of B prompts of UNEQUAL length in one forward: ids [B, T] right-padded with any valid token id, lengths [B] (host
        list or tensor, 1 <= L_b <= T) -> (last_logits [B, V] f32: the logits at every row's own last token, inference_params_dict).

        The padded batch runs through the ordinary cached-prefill forward once, its width rounded up to a multiple of `pad_to` (the columns
        added are filled with the row's last real token).  Every dense, norm and MLP launch is row-independent, attention and the Hyena
        operator are causal, and a pad is an ordinary token, so every activation is finite and positions t < L_b of row b are what a
        prefill of row b alone computes.  What the operator's one-T end state cannot give -- the modal state and FIR
        history at L_b - 1 -- comes from HipOps.hyena_state_at_zt.  The cache holds KV [B, T_pad, 2, H, hd] (rows >= L_b are pad keys: a
        decode that appends at its own position overwrites them), per-row FIR / modal states and `lengths` (device int64 [B]) on both
        records.  It is meant for per-row-position decode (`pos_tensor`, DecodePool); Generator's scalar seqlen_offset cannot describe it.
        A padding mask or an existing cache raises ValueError: a ragged batch starts at t = 0.  `kv_dtype`: the format of the KV cache
        returned ("fp8": DESIGN.md section 21)."""
        check_kv_dtype(kv_dtype)
        if padding_mask is not None or inference_params_dict is not None:
            raise ValueError("prefill_ragged: no padding_mask and no existing cache (a ragged batch starts at t = 0; pads are ordinary tokens)")
        if ids.dim() != 2:
            raise ValueError("input_ids must be [batch, length]")
        B, T = ids.shape
        lens = [int(n) for n in (lengths.tolist() if isinstance(lengths, torch.Tensor) else lengths)]
        if len(lens) != B or any(n < 1 or n > T for n in lens):
            raise ValueError(f"prefill_ragged: one length per row with 1 <= L_b <= T = {T}, got {lens}")
        pad_to = max(1, int(pad_to))
        Tw = (T + pad_to - 1) // pad_to * pad_to
        dev = self.device
        ids = ids.to(dev)
        lens_d = torch.tensor(lens, dtype=torch.int64, device=dev)
        if Tw != T:
            ids = torch.cat([ids, ids.gather(1, (lens_d - 1)[:, None]).expand(B, Tw - T)], dim=1)
        ipd = self.initialize_inference_params()
        ipd["mha"].max_batch_size = ipd["hyena"].max_batch_size = B
        ipd["mha"].max_seqlen = Tw
        ipd["mha"].lengths = ipd["hyena"].lengths = lens_d
        ipd["mha"].kv_dtype = kv_dtype
        h = self.hidden_states(ids.contiguous(), ipd)                                         # [B Tw, D]
        last = h.index_select(0, torch.arange(B, device=dev) * Tw + lens_d - 1).contiguous()   # only the B rows that are read
        logits = self.ops.linear(last, self.unembed.weight, None).view(B, self.vocab_size)
        return logits.float(), ipd

    @property
    def has_own_unembed(self) -> bool:
        """False once `model.unembed` has been replaced by another module (the identity-unembed embedding recipe)."""
        return isinstance(self.unembed, _Unembed)

    def unembed_rows(self, h: torch.Tensor, ipd) -> torch.Tensor:
        """The logits [rows, V] of final-norm rows h of a single-token step on the caches `ipd`: the row-invariant launch when the step
        is batch-invariant, the plain dense layer otherwise."""
        if ipd is not None and ipd["mha"].batch_invariant:
            return self.ops.linear_rowinv(h, self.unembed.weight, None)
        return self.ops.linear(h, self.unembed.weight, None)

    def _unembed_output(self, h: torch.Tensor, B: int, T: int) -> torch.Tensor:
        """What forward returns for the final-norm hidden states h [B T, D]: the logits [B, T, V], or -- with `model.unembed` replaced --
        whatever the replacement's unembed() makes of h [B, T, D] (upstream users swap in an identity module to get embeddings)."""
        if not self.has_own_unembed:
            return self.unembed.unembed(h.view(B, T, self.hidden_size))
        return self.ops.linear(h, self.unembed.weight, None).view(B, T, self.vocab_size)

    # ------------------------------------------------------------------ hipGraph-captured decode step
    # One decode step is ~270 short launches (the reference pays that per token too); at batch 1 the step is
    # launch-bound (5.2 ms against a 2.1 ms weight-streaming floor).  The step is therefore captured ONCE into a
    # hipGraph whose kernels read the token position from device memory, and replayed for every token.
    decode_graph = True          # set False (or EVO_AMD_DECODE_GRAPH=0) to run every decode step eagerly

    def _graph_eligible(self, ipd) -> bool:
        import os
        if not self.decode_graph or os.environ.get("EVO_AMD_DECODE_GRAPH", "1") == "0":
            return False
        if self.ops.name != "hip-gfx950" or self.ops.timer is not None:
            return False
        if not self.has_own_unembed:          # the captured step bakes in the engine's unembedding weight
            return False
        hy, mha = ipd["hyena"], ipd["mha"]
        if mha.kv_layout != "contiguous":     # a paged cache belongs to a decode pool, which captures its own step
            return False
        # every layer must already hold state (i.e. a prefill happened), on this device
        return all(i in hy.fir_state_dict for i in self.hyena_layer_idxs) and \
            all(i in mha.key_value_memory_dict for i in self.attn_layer_idxs)

    def _graph_decode_step(self, x, ipd):
        mha, hy = ipd["mha"], ipd["hyena"]
        B = x.shape[0]
        off = int(mha.seqlen_offset)
        st = self._dgraph
        cap = min(mha.key_value_memory_dict[i].shape[1] for i in self.attn_layer_idxs) if self.attn_layer_idxs else 1 << 62
        # The captured graph is bound to the ADDRESSES of the KV, modal-state and FIR-state tensors.  `st` keeps strong
        # references to the cache objects and to every captured tensor and compares by identity: a later cache can then
        # neither recycle a CPython id() nor a caching-allocator address of a freed buffer.
        same_bufs = (st is not None and st["B"] == B and st["mha"] is mha and st["hyena"] is hy and st["kv_dtype"] == mha.kv_dtype
                     and st["kv_layout"] == mha.kv_layout and st["weight_dtype"] == mha.weight_dtype
                     and st["batch_invariant"] == bool(mha.batch_invariant)
                     and all(mha.key_value_memory_dict.get(i) is t for i, t in st["kv"].items())
                     and all(hy.state_dict.get(i) is t for i, t in st["iir"].items())
                     and all(hy.fir_state_dict.get(i) is t for i, t in st["fir"].items()))
        if off + 1 > cap or not same_bufs:
            st = None
            self._dgraph = None                      # drops the references the stale graph held
            if off + 1 > cap or any(mha.key_value_memory_dict[i].shape[0] < B for i in self.attn_layer_idxs):
                for i in self.attn_layer_idxs:      # grow outside the graph, with headroom for the tokens to come
                    self._kv_buffer(mha, i, B, off + 1 + 4096, mha.key_value_memory_dict[i])
        try:
            if st is None:
                warm = self._dgraph_warm
                if warm is None or warm[0] is not mha or warm[1] is not hy or warm[2] != B:
                    self._dgraph_warm = (mha, hy, B)  # first step with these caches runs eagerly (warms M=B GEMMs)
                    return None
                dev = self.device
                st = {"B": B, "mha": mha, "hyena": hy, "kv_dtype": mha.kv_dtype, "kv_layout": mha.kv_layout,
                      "weight_dtype": mha.weight_dtype, "batch_invariant": bool(mha.batch_invariant),
                      "ids": torch.zeros(B, 1, dtype=torch.int64, device=dev),
                      "pos": torch.zeros(B, dtype=torch.int64, device=dev),
                      "kv": {i: mha.key_value_memory_dict[i] for i in self.attn_layer_idxs},
                      "iir": {i: hy.state_dict[i] for i in self.hyena_layer_idxs},
                      "fir": {i: hy.fir_state_dict[i] for i in self.hyena_layer_idxs}}
                st["ids"].copy_(x)
                st["pos"].fill_(off)
                mha.pos_tensor = st["pos"]
                self._row_index(B, dev)             # (allocated outside the capture)
                if mha.weight_dtype == "fp8":
                    self.prepare_fp8_weights()
                self._inv_freq(dev)
                g = torch.cuda.CUDAGraph()
                try:
                    with capture_graph(g):
                        h = self.hidden_states(st["ids"], ipd)
                        st["logits"] = self.unembed_rows(h, ipd).view(B, 1, self.vocab_size)
                        st["pos"].add_(1)
                finally:
                    mha.pos_tensor = None
                # the eager decode path updates every state in place; a capture that re-bound one would replay into a
                # buffer the cache no longer holds
                assert all(hy.state_dict[i] is t for i, t in st["iir"].items())
                assert all(hy.fir_state_dict[i] is t for i, t in st["fir"].items())
                st["graph"] = g
                st["next"] = off
                self._dgraph = st
            st["ids"].copy_(x)
            if st["next"] != off:
                st["pos"].fill_(off)
            st["graph"].replay()
            self.decode_graph_replays += 1
            st["next"] = off + 1
            return st["logits"].clone()
        except Exception as e:  # noqa: BLE001   capture is an optimisation: fall back to eager HIP launches
            import warnings
            warnings.warn(f"decode hipGraph disabled ({type(e).__name__}: {e}); continuing with eager launches")
            self.decode_graph = False
            self._dgraph = None
            return None

    def release_decode_graph(self):
        """Drop the captured decode step and the strong references it holds to the cache objects and to every KV / modal /
        FIR state tensor it was captured on (6.4 GB of KV cache after a 131k-context generation).  Called at the end of
        `Generator.generate` / `DecodePool.generate`; a later decode step on a live cache simply captures again."""
        self._dgraph = self._dgraph_warm = None

    # upstream names, kept for callers that reach for them
    def stateless_forward(self, x, padding_mask=None):
        return self.forward(x, None, padding_mask)

    def stateful_forward(self, x, inference_params_dict=None):
        return self.forward(x, inference_params_dict)
