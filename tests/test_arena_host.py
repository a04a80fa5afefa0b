"""CPU: the arena harness (tests/arena.py) tested on itself, with stand-in "kernels" written in torch on a CPU arena.

Four faulty stand-ins -- a store one element past the output's last row, a store into the band in front, a load of x[M] that reaches
a sum, a last output row that is never written -- must each fail with the right tensor and side named; the clean one must pass.
Plus the layout rules (address = 16 mod 32, band sizes, a strided tensor's pitch) and the proxy's routing.  This is what shows
without a GPU that a green run of tests/test_gpu_arena.py means something.

The stand-ins reach out of range the way a kernel does -- through the operand's base pointer.  On a fresh allocation the storage
ends with the tensor, so the stray access is dropped there (what allocator slack does for a real kernel: nobody sees it); inside the
arena the storage is the arena and the access lands in a guard band."""
import types

import pytest
import torch

import arena as A
from arena import Arena, ArenaError, TorchProxy, run_in_arena

M, N = 5, 8


def _in_storage(t, so):
    return 0 <= so and (so + 1) * t.element_size() <= t.untyped_storage().nbytes()


def poke(t, elem_offset, value):
    so = t.storage_offset() + elem_offset
    if _in_storage(t, so):
        t.as_strided((1,), (1,), so).fill_(value)


def peek(t, elem_offset):
    so = t.storage_offset() + elem_offset
    return t.as_strided((1,), (1,), so).clone()[0] if _in_storage(t, so) else torch.zeros((), dtype=t.dtype)


mod = types.SimpleNamespace(torch=torch)           # the stand-in for evo_amd.ops: its `torch` is what the proxy replaces


def k_clean(x):
    y = mod.torch.empty(M, N, dtype=torch.float32, device=x.device)
    y.copy_(x * 2)
    return y


def k_store_past_end(x):
    y = mod.torch.empty(M, N, dtype=torch.float32, device=x.device)
    y.copy_(x * 2)
    poke(y, M * N, 1.0)                             # y[M][0]
    return y


def k_store_in_front(x):
    y = mod.torch.empty(M, N, dtype=torch.float32, device=x.device)
    y.copy_(x * 2)
    poke(y, -1, 1.0)                                # y[-1][N - 1]
    return y


def k_load_past_end(x):
    y = mod.torch.empty(M, N, dtype=torch.float32, device=x.device)
    y.copy_(x * 2)
    y[M - 1, 0] += peek(x, M * N)                   # x[M][0] reaches a sum
    return y


def k_last_row_unwritten(x):
    y = mod.torch.empty(M, N, dtype=torch.float32, device=x.device)
    y[:M - 1].copy_(x[:M - 1] * 2)
    return y


def k_inplace(x, state):
    state.add_(x)
    return None


def k_writes_read_only(x):
    y = k_clean(x)
    x[0, 0] = 3.0
    return y


def _x():
    return torch.arange(M * N, dtype=torch.float32).view(M, N)


def test_clean_kernel_passes_and_gets_poisoned_skewed_operands():
    run = run_in_arena(k_clean, {"x": _x()}, module=mod)
    assert torch.equal(run.got[0], _x() * 2) and torch.equal(run.want[0], run.got[0])
    assert run.inputs["x"].data_ptr() % 32 == 16 and run.got[0].data_ptr() % 32 == 16
    assert run.got[0].untyped_storage().data_ptr() == run.arena.buf.untyped_storage().data_ptr()     # the binding's output was carved too
    assert mod.torch is torch                                                                       # the proxy is gone again


def test_store_past_the_last_row_names_the_output_and_the_row():
    with pytest.raises(ArenaError, match=rf"guard band behind k_store_past_end:\d+ \({M}, {N}\).*first at \(row {M}, column 0\)"):
        run_in_arena(k_store_past_end, {"x": _x()}, module=mod)


def test_store_in_front_names_the_output_and_the_side():
    with pytest.raises(ArenaError, match=rf"guard band in front of k_store_in_front:\d+ .*first at \(row -1, column {N - 1}\)"):
        run_in_arena(k_store_in_front, {"x": _x()}, module=mod)


def test_load_past_the_end_that_reaches_a_sum_changes_the_bits():
    with pytest.raises(ArenaError, match=rf"returned tensor #0 .*1 of {M * N} elements differ, first at \({M - 1}, 0\).*arena nan"):
        run_in_arena(k_load_past_end, {"x": _x()}, module=mod)
    run_in_arena(k_load_past_end, {"x": _x()}, module=mod, poison=False)        # the diagnosis switch: without the poison it hides


def test_unwritten_output_row_is_found():
    with pytest.raises(ArenaError, match=rf"returned tensor #0 .*{N} of {M * N} elements differ, first at \({M - 1}, 0\).*last at \({M - 1}, {N - 1}\)"):
        run_in_arena(k_last_row_unwritten, {"x": _x()}, module=mod)


def test_in_out_operands_are_compared_and_read_only_ones_must_not_change():
    run = run_in_arena(k_inplace, {"x": _x(), "state": torch.ones(M, N)}, inout=["state"], module=mod)
    assert torch.equal(run.inputs["state"], _x() + 1) and torch.equal(run.fresh_inputs["state"], _x() + 1)
    with pytest.raises(ArenaError, match="read-only operand 'x'"):
        run_in_arena(k_writes_read_only, {"x": _x()}, module=mod)
    with pytest.raises(ArenaError, match="read-only operand 'state'"):
        run_in_arena(k_inplace, {"x": _x(), "state": torch.ones(M, N)}, module=mod)


def test_poison_reads_as_nan_and_minus_one_and_every_dtype_views_cleanly():
    ar = Arena(4 << 20)
    for dt in (torch.bfloat16, torch.float32, torch.complex64):
        t = ar.empty((3, 8), dt)
        assert bool(torch.isnan(torch.view_as_real(t) if t.is_complex() else t.float()).all()), dt
    for dt in (torch.int32, torch.int64):
        assert bool((ar.empty((5,), dt) == -1).all())
    assert bool((ar.empty((7,), torch.uint8) == 0xFF).all())
    ar.check()


def test_alignment_rule():
    ar = Arena(8 << 20)
    for k, dt in enumerate((torch.bfloat16, torch.float32, torch.int64, torch.complex64, torch.uint8, torch.int32)):
        t = ar.empty((k + 1, 3 + k), dt)
        assert t.data_ptr() % 32 == 16 and A.check_address(t.data_ptr())
    assert ar.empty((4,), torch.int32, align=4).data_ptr() % 8 == 4                  # an operand that needs only its element's alignment
    assert ar.empty((4, 512), torch.float32, align=64).data_ptr() % 128 == 64        # an operand the header asked more of: exactly that
    flat = Arena(1 << 20, skew=False)
    assert flat.empty((4, 4), torch.bfloat16).data_ptr() % 512 == 0                  # skew off: ordinary allocator alignment
    ar.check()


def test_band_size_rule_contiguous_and_strided():
    ar = Arena(16 << 20)
    small = ar.empty((10, 8), torch.bfloat16)                                         # pitch 16 B: 256 rows = 4 KiB -> the 64 KiB floor
    wide = ar.empty((3, 4096), torch.bfloat16)                                        # pitch 8 KiB: 256 rows = 2 MiB
    strided = ar.empty((10, 8), torch.bfloat16, strides=(1024, 1))                    # rows 2 KiB apart: 256 rows = 512 KiB
    vec = ar.empty((1000,), torch.float32)
    assert strided.shape == (10, 8) and strided.stride() == (1024, 1) and small.is_contiguous()
    want = {0: 64 * 1024, 1: 256 * 8192, 2: 256 * 2048, 3: 64 * 1024}
    prev_end = 0
    for i, r in enumerate(ar.records):
        assert r.front[0] == prev_end                                                 # no byte between two tensors that is neither tensor nor band
        assert r.front[1] - r.front[0] >= want[i] and r.back[1] - r.back[0] >= want[i], i
        assert r.front[1] == r.start and r.back[0] == r.end
        prev_end = r.back[1]
    assert ar.records[0].front[0] == 0 and ar.records[-1].back[1] <= ar.buf.numel()   # the arena begins and ends with a band
    assert ar.records[2].end - ar.records[2].start == (9 * 1024 + 8) * 2              # a strided tensor owns its whole extent
    # a store between two rows of the strided tensor is inside its extent (the packed parent's business); one pitch past its last row is not
    poke(strided, 10 * 1024, 1.0)
    with pytest.raises(ArenaError, match=r"guard band behind tensor2 .*first at \(row 10, column 0\)"):
        ar.check()


def test_parent_then_slice_gives_the_models_views():
    ar = Arena(4 << 20)
    qkv = ar.place(torch.randn(2, 5, 3, 2, 64).bfloat16(), name="qkv")
    k = qkv[:, :, 1]
    assert k.stride() == (5 * 3 * 128, 3 * 128, 64, 1) and k.data_ptr() % 16 == 0
    ar.check()


class _Counting:
    device_type = "cpu"

    def __init__(self):
        self.calls = []

    def empty(self, shape, dtype, device, name):
        self.calls.append((tuple(shape), dtype, name))
        return torch.empty(shape, dtype=dtype)


def test_proxy_routes_the_four_allocators_and_nothing_else():
    c = _Counting()
    p = TorchProxy(c)
    a = p.empty(3, 4, dtype=torch.bfloat16, device="cpu")
    b = p.empty((2, 5), dtype=torch.float32)
    e = p.empty_like(a)
    z = p.zeros(6, dtype=torch.int32, device="cpu")
    f = p.full((2, 3), 7.0, dtype=torch.float32, device="cpu")
    assert [s for s, _, _ in c.calls] == [(3, 4), (2, 5), (3, 4), (6,), (2, 3)]
    assert [d for _, d, _ in c.calls] == [torch.bfloat16, torch.float32, torch.bfloat16, torch.int32, torch.float32]
    assert all(n.startswith("test_proxy_routes_the_four_allocators_and_nothing_else:") for _, _, n in c.calls)
    assert bool((z == 0).all()) and bool((f == 7.0).all()) and a.dtype == e.dtype and b.shape == (2, 5)
    n = len(c.calls)
    p.ones(3), p.tensor([1, 2]), p.arange(4), p.randn(2, 2), p.zeros_like(a), p.full_like(a, 1.0), p.empty_strided((2, 2), (2, 1))
    p.empty(3, device="meta"), p.zeros(3, device="meta"), p.full((3,), 1.0, dtype=torch.float32, device="meta")   # another device: torch's own
    assert len(c.calls) == n
    assert isinstance(a, p.Tensor) and p.cuda is torch.cuda and p.bfloat16 is torch.bfloat16 and p.view_as_real is torch.view_as_real
    assert TorchProxy.ROUTED == ("empty", "empty_like", "zeros", "full")


def test_binding_side_allocations_size_the_arena_and_leave_with_the_context():
    released = []

    def k_ws(x):
        ws = mod.torch.zeros(2048, 64, dtype=torch.float32, device=x.device)          # 512 KiB workspace, 64 KiB bands
        ws[0, :N] = x[0]
        return k_clean(x) + ws[0, :N].sum()
    run = run_in_arena(k_ws, {"x": _x()}, module=mod, release=lambda: released.append(1))
    assert len(run.arena.records) == 3 and len(released) >= 2
    assert run.arena.buf.numel() >= 2048 * 64 * 4 + 6 * 64 * 1024
