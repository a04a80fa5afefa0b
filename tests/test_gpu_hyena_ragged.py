"""GPU (-m gpu): the per-row Hyena end state of a ragged batch (evo_hyena_state_at_zt, csrc/hyena_ragged.hip).

z^T is built with zt_from_rows(..., nan) -- NaN in every pad position of the layout -- and positions >= lens[b] of every row are set
to NaN as well: nothing there may reach an output.  Per row b:
  * the state against the fp64 oracle R.op_hyena(z[b:b+1, :L_b]) within 2e-5 x max|ref row| (the project's end-state bound; 1e-4 at
    131,072 tokens, as test_gpu_kernels.test_hyena_single_pass_131k_long_memory has it);
  * the state against the engine's own B = 1 end state, ops.hyena_prefill(z[b:b+1, :L_b], want_state=True), at the same bound;
  * fir_out bit-equal to the z rows L_b - 2, L_b - 1 (zeros where t < 0).
Shapes: the smallest lengths and the segment boundary (C = evo_amd.ops.HYENA_RAGGED_SEG), beyond two segments and the full row, more
rows than the machine has workgroup slots for one head, the real width, a long row, the long-memory length.  Out-of-range lens are
clamped.  The arena cases of the entry live here (tests/test_gpu_arena.py is not edited): `covers` registers them at import."""
import pytest
import torch

from evo_amd.ops import HYENA_RAGGED_SEG as C
from oracle import stripedhyena_ref as R
from test_gpu_arena import _run, covers, rnd
from test_gpu_arena import gen as dgen
from test_gpu_arena import hyena_params as arena_params
from test_gpu_kernels import DEV, bf, gen, hyena_params, ops          # noqa: F401  (`ops` is the module fixture)

pytestmark = pytest.mark.gpu


def _case(ops, B, T, D, H, lens, seed, tol=2e-5):
    assert len(lens) == B and T % 64 == 0
    fir_w, fir_b, poles, res, dskip = prm = hyena_params(D, seed)
    z = bf(torch.randn(B, T, 3 * D, generator=gen(seed + 1)))
    zn = z.clone()
    for b, n in enumerate(lens):
        zn[b, n:] = float("nan")
    zt = ops.zt_from_rows(zn.to(DEV), B, T, float("nan"))
    d = [t.to(DEV) for t in prm]
    st, fir = ops.hyena_state_at_zt(zt, B, T, torch.tensor(lens, dtype=torch.int64, device=DEV), d[0], d[1], d[2], H)
    torch.cuda.synchronize()
    assert st.shape == (B, D, 8) and st.dtype == torch.complex64 and fir.shape == (B, 3 * D, 2) and fir.dtype == torch.bfloat16
    st, fir = st.cpu().to(torch.complex128), fir.cpu()
    assert bool(torch.isfinite(torch.view_as_real(st)).all())
    worst = worst_self = 0.0
    for b, n in enumerate(lens):
        zb = z[b:b + 1, :n]
        _, ref = R.op_hyena(zb, *prm, H)
        top = float(ref.abs().max())
        err = float((st[b] - ref[0]).abs().max())
        _, own = ops.hyena_prefill(zb.to(DEV).contiguous(), *d, H, want_state=True)
        err_self = float((st[b] - own[0].cpu().to(torch.complex128)).abs().max())
        worst, worst_self = max(worst, err / top), max(worst_self, err_self / top)
        assert err <= tol * top, (b, n, err, top)
        assert err_self <= tol * top, (b, n, err_self, top)
        want = torch.zeros(3 * D, 2, dtype=torch.bfloat16)
        want[:, max(0, 2 - n):] = z[b, max(0, n - 2):n].t()
        assert torch.equal(fir[b].view(torch.int16), want.view(torch.int16)), (b, n)
    print(f"[{B} x {T} x {D}, lens {lens if B <= 6 else '...'}] state vs fp64: worst {worst:.2e} of the row's max; vs the B = 1 end state {worst_self:.2e}")


def test_smallest_lengths_and_the_segment_boundary(ops):
    _case(ops, 6, 704, 256, 2, [1, 2, 3, C - 1, C, C + 1], 11)


def test_beyond_two_segments_and_the_full_row(ops):
    _case(ops, 2, 704, 256, 2, [2 * C + 1, 704], 13)


def test_more_rows_than_workgroup_streams(ops):
    g = gen(17)
    lens = [1, 320, 8, 9, 255, 256, 257, 319] + torch.randint(1, 321, (32,), generator=g).tolist()
    _case(ops, 40, 320, 128, 1, lens, 17)


def test_real_width(ops):
    _case(ops, 2, 576, 4096, 32, [9, 576], 19)


def test_long_row(ops):
    _case(ops, 1, 8192, 128, 1, [8191], 23)


def test_long_memory_131k(ops):
    """|p| up to 0.99999: 512 segments combined in fp64."""
    _case(ops, 1, 131072, 128, 1, [131071], 62, tol=1e-4)


def test_lens_out_of_range_are_clamped(ops):
    B, T, D, H = 2, 704, 256, 2
    fir_w, fir_b, poles, _, _ = [t.to(DEV) for t in hyena_params(D, 29)]
    zt = ops.zt_from_rows(bf(torch.randn(B, T, 3 * D, generator=gen(30))).to(DEV), B, T, float("nan"))
    run = lambda lens: ops.hyena_state_at_zt(zt, B, T, torch.tensor(lens, dtype=torch.int64, device=DEV), fir_w, fir_b, poles, H)
    st0, fir0 = run([1, T])
    st1, fir1 = run([0, T + 5])
    st2, fir2 = run([-7, 1 << 40])
    assert bool(torch.isfinite(torch.view_as_real(st0)).all())
    for st, fir in ((st1, fir1), (st2, fir2)):
        assert torch.equal(torch.view_as_real(st), torch.view_as_real(st0)) and torch.equal(fir.view(torch.int16), fir0.view(torch.int16))


def test_token_major_entry_is_the_same_kernel(ops):
    """hyena_state_at (the modal routing's entry): z [B, T, 3 D] with T that is no multiple of 64 -- bit for bit what the channel-major entry
    gives on the padded layout."""
    B, T, D, H = 3, 300, 256, 2
    lens = [300, 1, 257]
    fir_w, fir_b, poles, _, _ = [t.to(DEV) for t in hyena_params(D, 31)]
    z = bf(torch.randn(B, T, 3 * D, generator=gen(32))).to(DEV)
    st, fir = ops.hyena_state_at(z, lens, fir_w, fir_b, poles, H)
    zp = torch.full((B, 320, 3 * D), float("nan"), dtype=torch.bfloat16, device=DEV)
    zp[:, :T] = z
    st2, fir2 = ops.hyena_state_at_zt(ops.zt_from_rows(zp, B, 320, float("nan")), B, 320, lens, fir_w, fir_b, poles, H)
    assert torch.equal(torch.view_as_real(st), torch.view_as_real(st2)) and torch.equal(fir.view(torch.int16), fir2.view(torch.int16))
    assert bool(torch.isfinite(torch.view_as_real(st)).all())


# ================================================================================================ arena
@covers("evo_hyena_state_at_zt")
@pytest.mark.parametrize("B,T,D,H,lens", [(3, 704, 256, 2, [1, C + 1, 704]), (40, 320, 128, 1, None), (1, 1003, 128, 1, [1003]),
                                          (1, 1003, 128, 1, [999])])
def test_arena_state_at_zt(B, T, D, H, lens):
    """z^T, lens (an int64 vector: 8 (mod 16)), the parameters, and the workspace / state / history the binding allocates, carved from
    the poisoned arena; NaN in the pad positions.  1 x 1,003: the 16-byte group that holds the last token reaches into the pad positions."""
    from evo_amd.ops import default_ops
    ops, g = default_ops(), dgen(B + T)
    prm = arena_params(D, T + 1)
    if lens is None:
        lens = [1 + (37 * b) % T for b in range(B)]
    inp = dict(zt=ops.zt_from_rows(rnd((B, T, 3 * D), g), B, T, float("nan")), lens=torch.tensor(lens, dtype=torch.int64, device=DEV),
               fir_w=prm["fir_w"], fir_b=prm["fir_b"], poles=prm["poles"])
    run = _run(lambda zt, lens, fir_w, fir_b, poles: ops.hyena_state_at_zt(zt, B, T, lens, fir_w, fir_b, poles, H), inp,
               expect=["evo_hyena_state_at_zt"])
    assert run is not None


@covers("evo_hyena_state_at_zt")
def test_arena_state_at_token_major():
    from evo_amd.ops import default_ops
    ops, g = default_ops(), dgen(77)
    B, T, D, H = 3, 300, 256, 2
    prm = arena_params(D, 78)
    inp = dict(z=rnd((B, T, 3 * D), g), lens=torch.tensor([300, 2, 150], dtype=torch.int64, device=DEV), fir_w=prm["fir_w"],
               fir_b=prm["fir_b"], poles=prm["poles"])
    _run(lambda z, lens, fir_w, fir_b, poles: ops.hyena_state_at(z, lens, fir_w, fir_b, poles, H), inp, expect=["evo_hyena_state_at_zt"])
