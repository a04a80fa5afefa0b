"""Arena harness: run a call once on fresh allocations and once inside a poisoned arena, and demand the same bits.

What the value-parity tests cannot see is where a kernel reads and writes.  Their operands are fresh torch allocations (512-byte
aligned, rounded up in size, on the default stream): a store a few rows past y[M] lands in allocator slack, a load past x[M] reads
stale finite data, a launch on the wrong stream is ordered anyway.  Every kernel of libevo_mi355x.so is free of float atomics, so a
launch is a pure function of its operands' bits -- which makes the sharp test possible:

    want = fn(fresh clones)                        ordinary allocations, current stream
    got  = fn(the same data carved out of ONE uint8 tensor filled with 0xFF), on a side stream behind a filler
    want == got bit for bit, read-only inputs unchanged, and every byte of the arena that belongs to no tensor still 0xFF

0xFF in every byte reads as NaN in bf16 / f32 / c64 and as -1 in int32 / int64: a load past an operand's end that reaches a sum poisons
the result, a store past it damages a guard band.

Layout.  Every carved tensor has a guard band in front and one behind that belong to no tensor (two neighbours never share one): at
least `GBM` = 256 rows of that tensor at its own row pitch (256 = the largest tile any kernel here walks) and at least 64 KiB.  The
arena begins and ends with a band, so an overrun of less than one band in either direction stays inside the allocation: these tests
cannot cause a fault by construction.

Alignment.  The first byte of every carved tensor sits at an address that is 16 (mod 32): 16-byte aligned and NOT 32-byte aligned.
That is the weakest alignment a call site of evo_amd/ produces -- read from the call sites: sh/model.py and ops.py hand the kernels row
slices of bf16 matrices whose rows are whole multiples of 16 bytes (`x[M - r:]`, `res[Mm:]`, `xp[Mp:Mp + B r]`, `y[Mm:]`: D, N, K are
multiples of 8 elements), whole 128 KiB blocks of z^T (`zt[-1]`), and the q / k / v thirds of a packed qkv or of the KV cache
(`qkv[:, :, 1]`, `kv[:, :T, 0]`: offsets of H * hd * 2 bytes, hd in {64, 128}); f32 / int64 vectors (poles, rotary tables, positions,
ranges, rstd) are passed whole.  No call site slices inside a group of 8 bf16 elements, and include/evo_mi355x.h asks for 16 bytes
("Conventions"), so 16 (mod 32) is both the weakest alignment the product produces and exactly what the header demands.  The
exceptions, stated in the header: integer vectors -- the model embeds `input_ids[b0:b0 + nb]`, rows of 8 T bytes of an int64 matrix: 8-byte
aligned and no more -- which the cases carve with `align=8`, and the sampler's per-row vectors -- DecodePool.fill samples ONE slot through `s_top_k[slot:slot + 1]`,
`s_count[slot:slot + 1]`, ...: element alignment only -- which the sampler case carves with `align=` the element size (address =
align mod 2 align).  An operand for which the header demanded MORE than 16 bytes would get exactly that through the same argument.

Binding-side allocations.  Inside the arena context `evo_amd.ops`' own torch.empty / empty_like / zeros / full carve from the arena
too (a proxy object replaces the module's `torch` global; everything else is delegated to torch), so the outputs and workspaces
the binding allocates itself -- part_o, part_ml, vt, agg, ss, rstd, the split-K ws, the pool strips -- have bands as well and start out
as NaN.  In the fresh run the same proxy fills them with byte 0x55 instead, so an output element that no launch writes differs between
the two runs: "every element of the output was written" falls out of the bitwise comparison.

Diagnosis.  `run_in_arena(..., skew=, poison=, side_stream=)` switch the three ingredients off one at a time: skew=False carves at
512-byte boundaries, poison=False fills the arena with zeros, side_stream=False runs on the current stream without the filler.

A plain module (imported as `from arena import ...`; tests/ is on sys.path): no fixtures, no pytest settings.
"""
from __future__ import annotations

import contextlib
import sys
from typing import Callable, Dict, Iterable, List, Optional, Sequence

import torch

POISON = 0xFF
FRESH_FILL = 0x55
GBM = 256
MIN_BAND = 64 * 1024


class ArenaError(AssertionError):
    pass


def _itemsize(dtype) -> int:
    return torch.empty(0, dtype=dtype).element_size()


def _contiguous_strides(shape: Sequence[int]) -> List[int]:
    st, acc = [], 1
    for n in reversed(shape):
        st.append(acc)
        acc *= max(int(n), 1)
    return list(reversed(st))


def row_pitch_bytes(shape: Sequence[int], strides: Sequence[int], dtype) -> int:
    """Bytes between two rows of the tensor: the stride of its second-to-last dimension (a 1-D tensor: one element per row)."""
    it = _itemsize(dtype)
    if len(shape) >= 2 and int(strides[-2]) > 0:
        return int(strides[-2]) * it
    return it


def band_bytes(shape: Sequence[int], strides: Sequence[int], dtype) -> int:
    """Size of each of a tensor's two guard bands: >= GBM rows at its own pitch and >= 64 KiB, a multiple of 32."""
    b = max(MIN_BAND, GBM * row_pitch_bytes(shape, strides, dtype))
    return (b + 31) // 32 * 32


def _extent_elems(shape: Sequence[int], strides: Sequence[int]) -> int:
    if any(int(n) == 0 for n in shape):
        return 0
    return 1 + sum((int(n) - 1) * int(s) for n, s in zip(shape, strides))


def footprint(shape, strides, dtype, align: int = 16) -> int:
    """Upper bound of the arena bytes one carved tensor takes (two bands, the tensor, alignment slack)."""
    strides = _contiguous_strides(shape) if strides is None else strides
    return 2 * band_bytes(shape, strides, dtype) + _extent_elems(shape, strides) * _itemsize(dtype) + 4 * max(align, 512) + 64


def check_address(addr: int, align: int = 16) -> bool:
    """The arena's alignment rule: a multiple of `align` and not of 2 * align."""
    return addr % (2 * align) == align


class _Record:
    __slots__ = ("name", "shape", "strides", "dtype", "start", "end", "front", "back", "pitch", "itemsize")

    def __repr__(self):
        return f"{self.name} {tuple(self.shape)} {self.dtype}"


class Arena:
    """One uint8 tensor filled with `fill`; tensors are carved out of it front to back, each between two guard bands."""

    def __init__(self, capacity: int, device="cpu", skew: bool = True, poison: bool = True):
        self.fill = POISON if poison else 0x00
        self.skew = skew
        self.buf = torch.empty(int(capacity) + 1024, dtype=torch.uint8, device=device)
        self.buf.fill_(self.fill)
        self.base = self.buf.data_ptr()
        self.cursor = 0
        self.records: List[_Record] = []

    @property
    def device(self):
        return self.buf.device

    def empty(self, shape, dtype, strides=None, align: int = 16, name: Optional[str] = None) -> torch.Tensor:
        """An uninitialised (= still poisoned) tensor of exactly this shape, dtype and strides (default: contiguous)."""
        shape = [int(n) for n in shape]
        strides = _contiguous_strides(shape) if strides is None else [int(s) for s in strides]
        if any(s < 0 for s in strides):
            raise ValueError("arena: negative strides")
        it = _itemsize(dtype)
        nbytes = _extent_elems(shape, strides) * it
        band = band_bytes(shape, strides, dtype)
        start = self.cursor + band
        if self.skew:                                        # address = align (mod 2 align): aligned to `align` and to nothing more
            start += (align - (self.base + start)) % (2 * align)
        else:
            start += (-(self.base + start)) % 512
        end = start + nbytes
        new_cursor = (end + band + 31) // 32 * 32
        if new_cursor > self.buf.numel():
            raise ArenaError(f"arena of {self.buf.numel()} bytes is full: {name or 'tensor'} {tuple(shape)} needs {new_cursor - self.cursor} more")
        r = _Record()
        r.name = name or f"tensor{len(self.records)}"
        r.shape, r.strides, r.dtype, r.itemsize = shape, strides, dtype, it
        r.start, r.end = start, end
        r.front, r.back = (self.cursor, start), (end, new_cursor)
        r.pitch = row_pitch_bytes(shape, strides, dtype)
        self.records.append(r)
        self.cursor = new_cursor
        flat = self.buf[start:end].view(dtype) if nbytes else torch.empty(0, dtype=dtype, device=self.device)
        return flat.as_strided(shape, strides)

    def place(self, t: torch.Tensor, align: int = 16, name: Optional[str] = None) -> torch.Tensor:
        """A copy of t inside the arena with t's shape, dtype and strides.  Non-contiguous layouts the way the model builds them: place
        the packed parent, then slice."""
        v = self.empty(t.shape, t.dtype, None if t.is_contiguous() else t.stride(), align=align, name=name)
        v.copy_(t)
        return v

    def _where(self, r: _Record, byte: int):
        d = byte - r.start
        return d // r.pitch, (d % r.pitch) // r.itemsize

    def damage(self) -> List[str]:
        """One line per damaged band: the tensor it belongs to, the side, first and last damaged byte as (row, column) of that tensor."""
        out = []
        spans = []
        for r in self.records:
            spans.append((r, "in front of", r.front))
            spans.append((r, "behind", r.back))
        if self.records:
            spans.append((self.records[-1], "in the unclaimed space behind", (self.cursor, self.buf.numel())))
        for r, side, (lo, hi) in spans:
            if hi <= lo:
                continue
            bad = self.buf[lo:hi] != self.fill
            if bool(bad.any()):
                idx = bad.nonzero().flatten()
                first, last = lo + int(idx[0]), lo + int(idx[-1])
                (r0, c0), (r1, c1) = self._where(r, first), self._where(r, last)
                out.append(f"guard band {side} {r!r} damaged: {idx.numel()} bytes, first at (row {r0}, column {c0}), last at (row {r1}, "
                           f"column {c1}) of its pitch of {r.pitch} bytes [{r.shape[0] if r.shape else 1} rows; byte {first - r.start:+d} .. "
                           f"{last - r.start:+d} from its first byte]")
        return out

    def check(self) -> None:
        """Every band is still all fill bytes, compared as uint8."""
        msgs = self.damage()
        if msgs:
            raise ArenaError("\n".join(msgs))


# ---- the proxy that replaces `torch` in evo_amd.ops (and in the host tests' stand-in module) --------------------------------------------
class _FreshAllocator:
    """The fresh run: ordinary torch allocations, filled with byte 0x55 (an element nobody writes then differs from the arena run's
    0xFF); records what was asked for, so that the arena can be sized."""

    def __init__(self, device_type: str):
        self.device_type = device_type
        self.log = []

    def empty(self, shape, dtype, device, name):
        t = torch.empty(shape, dtype=dtype, device=device)
        if t.numel():
            t.view(-1).view(torch.uint8).fill_(FRESH_FILL)
        self.log.append((list(shape), dtype))
        return t


class _ArenaAllocator:
    def __init__(self, arena: Arena):
        self.arena = arena
        self.device_type = arena.device.type

    def empty(self, shape, dtype, device, name):
        return self.arena.empty(shape, dtype, name=name)


def _shape_of(size) -> List[int]:
    if len(size) == 1 and isinstance(size[0], (tuple, list, torch.Size)):
        size = size[0]
    return [int(n) for n in size]


class TorchProxy:
    """Stands in for the `torch` module: empty / empty_like / zeros / full for tensors on the allocator's device go to the allocator,
    every other attribute is torch's own."""

    ROUTED = ("empty", "empty_like", "zeros", "full")

    def __init__(self, allocator):
        self._allocator = allocator

    def __getattr__(self, name):
        return getattr(torch, name)

    def _mine(self, device) -> bool:
        return torch.device("cpu" if device is None else device).type == self._allocator.device_type

    @staticmethod
    def _caller() -> str:
        f = sys._getframe(2)
        return f"{f.f_code.co_name}:{f.f_lineno}"

    def empty(self, *size, dtype=None, device=None, **kw):
        if kw or not self._mine(device):
            return torch.empty(*size, dtype=dtype, device=device, **kw)
        return self._allocator.empty(_shape_of(size), dtype or torch.get_default_dtype(), device, self._caller())

    def empty_like(self, t, **kw):
        if kw or not self._mine(t.device) or not t.is_contiguous():
            return torch.empty_like(t, **kw)
        return self._allocator.empty(list(t.shape), t.dtype, t.device, self._caller())

    def zeros(self, *size, dtype=None, device=None, **kw):
        if kw or not self._mine(device):
            return torch.zeros(*size, dtype=dtype, device=device, **kw)
        return self._allocator.empty(_shape_of(size), dtype or torch.get_default_dtype(), device, self._caller()).zero_()

    def full(self, size, fill_value, dtype=None, device=None, **kw):
        if kw or dtype is None or not self._mine(device):
            return torch.full(size, fill_value, dtype=dtype, device=device, **kw)
        return self._allocator.empty(_shape_of((size,)), dtype, device, self._caller()).fill_(fill_value)


@contextlib.contextmanager
def patched_torch(module, allocator):
    """`module.torch` is a TorchProxy on `allocator` inside the block."""
    if module is None:
        yield None
        return
    real = module.torch
    proxy = TorchProxy(allocator)
    module.torch = proxy
    try:
        yield proxy
    finally:
        module.torch = real


# ---- bitwise comparison -----------------------------------------------------------------------------------------------------------------
def bits(t: torch.Tensor) -> torch.Tensor:
    """The tensor's bytes as a uint8 tensor [numel, itemsize] (NaN cannot hide a difference)."""
    if t.is_complex():
        t = torch.view_as_real(t)
    if t.dtype == torch.bool:
        t = t.to(torch.uint8)
    t = t.contiguous()
    return t.view(-1).view(torch.uint8).view(t.numel(), -1) if t.numel() else t.view(-1).view(torch.uint8).view(0, 1)


def first_difference(a: torch.Tensor, b: torch.Tensor) -> Optional[str]:
    """None when a and b hold the same bits, else where they first and last differ (index in the tensor's shape)."""
    if a.shape != b.shape or a.dtype != b.dtype:
        return f"shape / dtype differ: {tuple(a.shape)} {a.dtype} vs {tuple(b.shape)} {b.dtype}"
    ba, bb = bits(a), bits(b)
    if torch.equal(ba, bb):
        return None
    bad = (ba != bb).any(-1).nonzero().flatten()
    ref = torch.view_as_real(a) if a.is_complex() else a
    shape = list(ref.shape)

    def at(flat):
        idx = []
        for n in reversed(shape):
            idx.append(flat % n)
            flat //= n
        return tuple(reversed(idx))
    i0, i1 = int(bad[0]), int(bad[-1])
    fa, fb = ref.contiguous().view(-1), (torch.view_as_real(b) if b.is_complex() else b).contiguous().view(-1)
    return (f"{bad.numel()} of {ba.shape[0]} elements differ, first at {at(i0)} (fresh {fa[i0].item()!r}, arena {fb[i0].item()!r}), "
            f"last at {at(i1)} (fresh {fa[i1].item()!r}, arena {fb[i1].item()!r})")


def _flatten(out) -> List[torch.Tensor]:
    if out is None:
        return []
    if isinstance(out, torch.Tensor):
        return [out]
    if isinstance(out, dict):
        out = list(out.values())
    res = []
    for o in out:
        res.extend(_flatten(o))
    return res


# ---- the filler behind which the arena run is enqueued --------------------------------------------------------------------------------
_FILLER = {}


def _enqueue_filler(device) -> None:
    """A multi-millisecond matmul on scratch tensors on the current stream (fp32 8192 x 4096 x 8192: 0.55 Tflop)."""
    key = str(device)
    if key not in _FILLER:
        a = torch.randn(8192, 4096, device=device)
        b = torch.randn(4096, 8192, device=device)
        _FILLER[key] = (a, b, torch.empty(8192, 8192, device=device))
    a, b, c = _FILLER[key]
    torch.mm(a, b, out=c)


class ArenaRun:
    """What run_in_arena hands back for further assertions: `want` / `got` = the returned tensors of the fresh / arena run, `inputs` =
    the arena's operands after the call (by name), `fresh_inputs` = the fresh run's, `arena` = the Arena (bands already checked)."""

    def __init__(self, want, got, inputs, fresh_inputs, arena):
        self.want, self.got, self.inputs, self.fresh_inputs, self.arena = want, got, inputs, fresh_inputs, arena


def run_in_arena(fn: Callable, inputs: Dict[str, torch.Tensor], inout: Iterable[str] = (), module=None,
                 release: Optional[Callable[[], None]] = None, skew: bool = True, poison: bool = True, side_stream: bool = True,
                 align: Optional[Dict[str, int]] = None, device=None, slack: int = 1 << 20) -> ArenaRun:
    """fn(**inputs) once on fresh clones and once inside a poisoned arena; asserts equal bits for every returned tensor and every
    operand, unchanged read-only operands (every name not in `inout`) and intact guard bands.  `inputs`: contiguous tensors by name
    (views are made inside fn: place the packed parent, then slice); `module`: the module whose `torch` global the proxy replaces
    (evo_amd.ops); `release`: called when leaving each context (ops.release_workspaces: cached workspaces must not outlive the arena)."""
    inout = set(inout)
    align = dict(align or {})
    assert inout <= set(inputs), f"inout names {inout - set(inputs)} are not inputs"
    for k, t in inputs.items():
        assert t.is_contiguous(), f"input {k}: place the packed parent and slice inside fn"
    if device is None:
        device = next(iter(inputs.values())).device if inputs else torch.device("cpu")
    device = torch.device(device)
    on_gpu = device.type == "cuda"
    release = release or (lambda: None)

    # 1. fresh allocations, current stream
    fresh = {k: t.clone() for k, t in inputs.items()}
    rec = _FreshAllocator(device.type)
    release()
    with patched_torch(module, rec):
        try:
            want = _flatten(fn(**fresh))
        finally:
            release()
    if on_gpu:
        torch.cuda.synchronize(device)
    for k, t in inputs.items():
        if k not in inout:
            d = first_difference(t, fresh[k])
            if d:
                raise ArenaError(f"fresh run changed the read-only operand '{k}': {d}")

    # 2. the arena: sized from the operands and from what the binding allocated in the fresh run
    need = slack + sum(footprint(t.shape, None, t.dtype, align.get(k, 16)) for k, t in inputs.items())
    need += sum(footprint(shape, None, dtype) for shape, dtype in rec.log)
    arena = Arena(need, device=device, skew=skew, poison=poison)
    carved = {k: arena.empty(t.shape, t.dtype, align=align.get(k, 16), name=k) for k, t in inputs.items()}
    if skew:
        for k, v in carved.items():
            assert v.numel() == 0 or check_address(v.data_ptr(), align.get(k, 16)), (k, hex(v.data_ptr()))

    def body():
        for k, t in inputs.items():                           # until these copies run the carved operands hold the poison
            carved[k].copy_(t)
        with patched_torch(module, _ArenaAllocator(arena)):
            try:
                return _flatten(fn(**carved))
            finally:
                release()

    if on_gpu and side_stream:
        side = torch.cuda.Stream(device=device)
        side.wait_stream(torch.cuda.current_stream(device))   # (the arena's fill ran on the current stream)
        with torch.cuda.stream(side):
            _enqueue_filler(device)
            got = body()
        side.synchronize()
        torch.cuda.synchronize(device)
    else:
        got = body()
        if on_gpu:
            torch.cuda.synchronize(device)

    # 3. the same bits, read-only operands unchanged, bands intact
    problems = []
    if len(want) != len(got):
        problems.append(f"fresh run returned {len(want)} tensors, arena run {len(got)}")
    for i, (a, b) in enumerate(zip(want, got)):
        d = first_difference(a, b)
        if d:
            problems.append(f"returned tensor #{i} {tuple(a.shape)} {a.dtype}: {d}")
    for k in inputs:
        d = first_difference(fresh[k], carved[k])
        if d:
            problems.append(f"operand '{k}' after the call: {d}")
        if k not in inout:
            d = first_difference(inputs[k], carved[k])
            if d:
                problems.append(f"read-only operand '{k}' changed in the arena run: {d}")
    problems.extend(arena.damage())
    if problems:
        raise ArenaError("\n".join(problems))
    return ArenaRun(want, got, carved, fresh, arena)
