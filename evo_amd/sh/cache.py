"""`stripedhyena.cache` mirror: the two cache records evo's generation loop reads and mutates
[REF evo/generation.py:105-120,138-148]."""
from dataclasses import dataclass, field
from typing import Optional

import torch
from torch import Tensor


@dataclass
class SharedPrefix:
    """Keys / values of ONE reference sequence that every row of a batch continues (evo_amd.scoring.score_variants):
    kv[layer] = the reference's own KV buffer [1, cap, 2, H, hd] (read through views, never copied or expanded),
    vt[layer] = its V^T plane [H, hd, cols] for HipOps.attention_prefix (absent on backends that need none)."""
    kv: dict = field(default_factory=dict)
    vt: dict = field(default_factory=dict)


@dataclass
class PromptStore:
    """Keys / values of the PROMPTS a decode pool samples from, one stored copy per live prompt (evo_amd.pool.DecodePool with
    share_prompt_kv): kv[layer] = [R, P_cap, 2, H, hd]; row [S]: the store row slot s continues (-1: none); length [R]: the keys a
    store row holds; own_pos [S]: the index of the slot's current token in its OWN cache (its absolute position minus the prompt's
    length).  All three vectors are device int64, so a captured step replays unchanged while slots are re-filled."""
    kv: dict = field(default_factory=dict)
    row: Optional[Tensor] = None
    length: Optional[Tensor] = None
    own_pos: Optional[Tensor] = None


KV_DTYPES = ("bf16", "fp8")


def check_kv_dtype(kv_dtype) -> str:
    """`kv_dtype` if it names a cache format; ValueError otherwise (raised before any device work)."""
    if kv_dtype not in KV_DTYPES:
        raise ValueError(f"kv_dtype must be one of {KV_DTYPES}, got {kv_dtype!r}")
    return kv_dtype


@dataclass(eq=False)
class Fp8KV:
    """One attention layer's FP8 (e4m3fn) KV cache: data [B, cap, 2, H, 128] uint8 -- the bf16 cache's layout,
    byte-wide -- and scale [B, 2, H, cap] f32, one power of two per cached row (token-contiguous per head).  The value of
    key_value_memory_dict[layer] when InferenceParams.kv_dtype == "fp8"; compared by identity, like the tensor it stands for."""
    data: Tensor
    scale: Tensor

    @classmethod
    def zeros(cls, B: int, cap: int, H: int, hd: int, device) -> "Fp8KV":
        return cls(torch.zeros(B, cap, 2, H, hd, dtype=torch.uint8, device=device), torch.ones(B, 2, H, cap, dtype=torch.float32, device=device))

    @property
    def shape(self):
        return self.data.shape

    @property
    def device(self):
        return self.data.device

    def nbytes(self) -> int:
        return self.data.numel() * self.data.element_size() + self.scale.numel() * self.scale.element_size()

    def to(self, device) -> "Fp8KV":
        return self if self.data.device == device else Fp8KV(self.data.to(device), self.scale.to(device))

    def rows(self, B: int) -> "Fp8KV":
        """The first B batch rows, as views."""
        return Fp8KV(self.data[:B], self.scale[:B])

    def copy_rows_(self, dst_b, src: "Fp8KV", src_b, n: int) -> None:
        """Tokens [0, n) of batch row(s) `src_b` of `src` -> the same tokens of batch row(s) `dst_b` of this cache."""
        self.data[dst_b, :n] = src.data[src_b, :n]
        self.scale[dst_b, :, :, :n] = src.scale[src_b, :, :, :n]

    def dequantize(self) -> Tensor:
        """[B, cap, 2, H, 128] f32: byte * scale, exact."""
        return self.data.view(torch.float8_e4m3fn).float() * self.scale.permute(0, 3, 1, 2).unsqueeze(-1)


KV_LAYOUTS = ("contiguous", "paged")
KV_PAGE_TOKENS_MIN = 64     # a 64-key block of the streaming decode attention must lie inside one page


def check_page_tokens(page_tokens) -> int:
    """`page_tokens` if it is a power of two >= 64; ValueError otherwise (raised before any device work)."""
    n = int(page_tokens)
    if n < KV_PAGE_TOKENS_MIN or n & (n - 1):
        raise ValueError(f"kv_page_tokens must be a power of two >= {KV_PAGE_TOKENS_MIN}, got {page_tokens!r}")
    return n


@dataclass(eq=False)
class PagedKV:
    """One attention layer's paged bf16 KV cache: pages [n_pages, page_tokens, 2, H, 128] -- a page is a
    [page_tokens, 2, H, 128] view with the contiguous cache's inner layout -- and table [n_slots, table_width] int32 on the device, ONE
    tensor shared by every attention layer of a pool: token t of slot s lives in pages[table[s, t // page_tokens], t % page_tokens].
    Page 0 is a scrap page that is never handed out; every table entry no live job owns holds 0.  The value of
    key_value_memory_dict[layer] when InferenceParams.kv_layout == "paged"; compared by identity."""
    pages: Tensor
    table: Tensor

    @classmethod
    def zeros(cls, n_pages: int, page_tokens: int, H: int, hd: int, table: Tensor, dtype=torch.bfloat16) -> "PagedKV":
        check_page_tokens(page_tokens)
        return cls(torch.zeros(n_pages, page_tokens, 2, H, hd, dtype=dtype, device=table.device), table)

    @property
    def page_tokens(self) -> int:
        return self.pages.shape[1]

    @property
    def n_pages(self) -> int:
        return self.pages.shape[0]

    @property
    def table_width(self) -> int:
        return self.table.shape[1]

    @property
    def shape(self):
        return self.pages.shape

    @property
    def device(self):
        return self.pages.device

    def nbytes(self) -> int:
        """Bytes of the page pool (the table is shared by all layers and a few KiB)."""
        return self.pages.numel() * self.pages.element_size()

    def rows(self, B: int) -> "PagedKV":
        """The first B table rows, as a view (the pages are the pool's)."""
        return self if self.table.shape[0] == B else PagedKV(self.pages, self.table[:B])

    def write_tokens_(self, page_ids: Tensor, src: Tensor) -> None:
        """src [n, 2, H, 128] -> tokens 0 .. n - 1 of the stream whose pages are `page_ids` (device int64, in order)."""
        n, pt = src.shape[0], self.page_tokens
        t = torch.arange(n, device=src.device)
        self.pages[page_ids[t // pt], t % pt] = src

    def gather(self, slot: int, n: int) -> Tensor:
        """Tokens 0 .. n - 1 of slot `slot` as one [n, 2, H, 128] tensor (tests, inspection: not a hot path)."""
        pt = self.page_tokens
        t = torch.arange(n, device=self.pages.device)
        return self.pages[self.table[slot].long()[t // pt], t % pt]


WEIGHT_DTYPES = ("bf16", "fp8")
W8_MAX_ROWS = 8        # batch rows the FP8-weight launches of a backend serve unless it declares more (Backend.W8_ROWS; csrc/gemv_fp8.hip: the dot2 forms)
W8_WIDE_K = 256        # above W8_MAX_ROWS rows every streamed layer's K is a multiple of this (csrc/skinny_fp8.hip: whole 256-k units)


def check_weight_dtype(weight_dtype) -> str:
    """`weight_dtype` if it names a format of the decode step's dense weights; ValueError otherwise (raised before any device work)."""
    if weight_dtype not in WEIGHT_DTYPES:
        raise ValueError(f"weight_dtype must be one of {WEIGHT_DTYPES}, got {weight_dtype!r}")
    return weight_dtype


def check_weight_rows(rows: int, what: str, max_rows: int = W8_MAX_ROWS) -> None:
    """ValueError when `rows` decode streams are more than the backend's FP8-weight launches serve (`max_rows`: its Backend.W8_ROWS)."""
    if rows > max_rows:
        why = " (the 9-64-row launches are bf16 only)" if max_rows == W8_MAX_ROWS else ""
        raise ValueError(f'weight_dtype="fp8" serves at most {max_rows} rows per decode step, got {what} = {rows}{why}')


ROWINV_MAX_ROWS = 64    # batch rows the row-invariant dense launches serve (csrc/gemv_inv.hip)
ROWINV_SPLITS = 32      # decode-attention splits of the batch-invariant step: what HipOps._decode_splits returns from 1,857 keys of capacity up


def check_rowinv_rows(rows: int, what: str) -> None:
    """ValueError when `rows` decode streams are more than the row-invariant launches serve."""
    if rows > ROWINV_MAX_ROWS:
        raise ValueError(f"batch_invariant=True serves at most {ROWINV_MAX_ROWS} rows per decode step, got {what} = {rows}")


def fp8_row_rule(w: Tensor):
    """THE RULE of the FP8 formats (include/evo_mi355x.h, ABI 19 / 20) in torch, on rows w [N, K]: with a = max |w[n, :]|, e is the smallest
    integer with a 2^-e <= 448, clamped to [-126, 120] (a = 0: e = 0) -> (bytes RNE_e4m3fn(w 2^-e) [N, K] uint8, scales 2^e [N] f32).
    e comes from frexp (exact), never from a logarithm; inputs are finite."""
    wf = w.float()
    a = wf.abs().amax(dim=1)
    m, ex = torch.frexp(a)                                   # a = m 2^ex, 0.5 <= m < 1;  448 = 0.875 * 2^9
    e = ex - 9 + (m > 0.875).to(ex.dtype)
    e = torch.where(a == 0, torch.zeros_like(e), e.clamp(-126, 120))
    data = (wf * torch.exp2(-e.float())[:, None]).to(torch.float8_e4m3fn).view(torch.uint8)
    return data, torch.exp2(e.float())


@dataclass(eq=False)
class Fp8Weight:
    """One dense weight of the decode step in FP8 e4m3fn: data [N, K] uint8 row-major and scale [N] f32, one power
    of two per output feature, by fp8_row_rule."""
    data: Tensor
    scale: Tensor

    @classmethod
    def quantize(cls, w: Tensor) -> "Fp8Weight":
        return cls(*fp8_row_rule(w))

    @property
    def shape(self):
        return self.data.shape

    @property
    def device(self):
        return self.data.device

    def nbytes(self) -> int:
        return self.data.numel() * self.data.element_size() + self.scale.numel() * self.scale.element_size()

    def dequantize(self, dtype=torch.bfloat16) -> Tensor:
        """[N, K]: byte * scale -- exact in fp32, and exact in bf16 (a byte has four significant bits, the scale is a power of two)."""
        return (self.data.view(torch.float8_e4m3fn).float() * self.scale[:, None]).to(dtype)


@dataclass
class InferenceParams:
    """Attention layers: key_value_memory_dict[layer] = [B_max, max_seqlen, 2, H, hd] bf16, or with kv_dtype == "fp8" an Fp8KV record."""
    max_seqlen: int
    max_batch_size: int
    seqlen_offset: int = 0
    batch_size_offset: int = 0
    key_value_memory_dict: dict = field(default_factory=dict)
    # "bf16" (default) or "fp8": the format of the KV cache (opt-in)
    kv_dtype: str = "bf16"
    # "contiguous" (default) or "paged": key_value_memory_dict[layer] is then a PagedKV record (opt-in, the decode pool's per-row step only;
    # DESIGN.md section 23)
    kv_layout: str = "contiguous"
    # "bf16" (default) or "fp8": the dense weights the single-token steps on this cache stream (opt-in).  Read for
    # the Hyena blocks of the step too: the choice belongs to the generation, and this record is the one every step carries
    weight_dtype: str = "bf16"
    # set: the single-token steps on this cache run ONE launch sequence whose arithmetic per row does not depend on the number of rows or
    # on the cache capacity (opt-in, the decode pool).  Like weight_dtype it is read for the Hyena blocks too
    batch_invariant: bool = False
    lengths_per_sample: Optional[Tensor] = None
    # set: the rows continue the first `seqlen_offset` tokens of a shared reference -- attention reads that prefix from shared_prefix.kv and
    # no per-row KV buffer is allocated or written (StripedHyena._attn_block)
    shared_prefix: Optional[SharedPrefix] = None
    # set (with pos_tensor, single-token steps): key_value_memory_dict holds only the tokens each row GENERATED; the prompt it continues is
    # read from prompt_store (StripedHyena._attn_block)
    prompt_store: Optional[PromptStore] = None
    # set by StripedHyena.prefill_ragged: device int64 [B], the tokens of every row of a right-padded batch that are real.  KV rows behind
    # lengths[b] hold pad keys (a per-row-position decode overwrites them as it appends); a scalar seqlen_offset cannot describe such a cache
    lengths: Optional[Tensor] = None
    # set for the duration of a single-token step (DecodePool, the captured decode step): device int64, one position PER ROW (or one for all)
    # -- rotary, the KV append and the decode attention read it instead of the scalar seqlen_offset
    pos_tensor: Optional[Tensor] = None
    # (cos, sin) of pos_tensor for all attention layers of ONE step, on backends without "rope_append_decode" (StripedHyena.hidden_states)
    _rot_dyn: Optional[tuple] = None

    def reset(self, max_seqlen, max_batch_size):
        self.max_seqlen = max_seqlen
        self.max_batch_size = max_batch_size
        self.seqlen_offset = 0
        if self.lengths_per_sample is not None:
            self.lengths_per_sample.zero_()


@dataclass
class RecurrentInferenceParams:
    """Hyena layers: fir_state_dict[layer] = [B, 3D, 2] (last two pre-FIR inputs, oldest first),
    state_dict[layer] = [B, D, 8] complex64 (modal state after the last token)."""
    fir_filter_length: int = 3
    state_dim: int = 16
    seqlen_offset: int = 0
    fir_state_dict: dict = field(default_factory=dict)
    state_dict: dict = field(default_factory=dict)
    max_batch_size: int = 1
    # ragged prefill (see InferenceParams.lengths): the states are those after token lengths[b] - 1 of row b
    lengths: Optional[Tensor] = None

    def reset(self):
        self.fir_filter_length = 3
        self.state_dim = 16
        self.seqlen_offset = 0
