"""CPU: the exact inputs of tests/hyena_fused_exact.py for the fused single-token Hyena launches are what they claim, on every (D, M, T)
that tests/test_gpu_hyena_fused_exact.py runs:

  * the RMSNorm of every token row is exact in fp32 statement by statement (dense_exact.rmsnorm_fp32_emulated): s / 2, inv = 2^-6;
  * the projection has one product per output, so norm(xs) W^T + b is exact in fp32 in any order of summation, and equals z after a bf16
    rounding that changes nothing; W is a fixed point of the FP8 rule (all-zero rows included);
  * z with the filter parameters satisfies its family's exactness conditions (hyena_exact.reference(..., check=...), asserted while the
    data set is built), for U with a tenth or more of the outputs rounded at the store and at least one exact tie, at every M;
  * the oracle's op_hyena_step, stepped on z from the start state, reproduces the reference's y, FIR history and modal state at EVERY step;
  * the defects the GPU module is there to catch differ from the reference under the module's own rule.

Which family sees which mutant of the single-token launches, in y (after the store's rounding), the FIR history or the modal state --
the same at every (D, M) of the table (state_prev_row needs M >= 2), asserted below against hyena_fused_exact.CAUGHT:
    mutant            U                   I
    state_prev_row    y, state            y, state    (the start states of two rows differ)
    chan_xor1         y, state            y, state    (I: neighbouring channels hold different poles by construction)
    fir_old_kept      y, state, fir       fir         (I's FIR reads no history: only fir_state shows it)
    state_early       state               state       (y is untouched)
"""
import pytest
import torch

import dense_exact as DX
import hyena_exact as X
import hyena_fused_exact as F
from evo_amd.backend import Backend
from evo_amd.sh.cache import Fp8Weight, fp8_row_rule
from oracle import stripedhyena_ref as R

CELLS = [(fam, D) for D, _ in F.SHAPES for fam in ("U", "I")]
_DATA = {}


def data(fam, D):
    if (fam, D) not in _DATA:
        _DATA[fam, D] = F.make(fam, D)                    # (asserts the family's conditions on the reference it returns)
    return _DATA[fam, D]


def test_shape_table():
    """The table holds every form of the launch: 4096 x 1 .. 8 (staged), 256 and 1024 x 1 .. 4 (unstaged), and each cell is one the
    fused launch accepts (Backend.fused_rows_ok; D = 128 heads)."""
    assert dict(F.SHAPES) == {4096: tuple(range(1, 9)), 256: (1, 2, 3, 4), 1024: (1, 2, 3, 4)}
    for D, Ms in F.SHAPES:
        assert D % 128 == 0 and 2 ** (D.bit_length() - 1) == D and (D.bit_length() - 1) % 2 == 0     # sqrt(D) a power of two
        assert all(Backend.fused_rows_ok(M, D) for M in Ms)
        assert not Backend.fused_rows_ok(max(Ms) + 1, D)
    assert F.U_STEPS == 40 and F.I_STEPS == 140 and F.I_IMPULSE_STEPS + 97 <= F.I_STEPS
    assert sorted(F.CAUGHT) == sorted(F.MUTANTS) and set(F.MUTANTS) <= {n for n, _ in X.mutants()}


@pytest.mark.parametrize("n", [0, 1, 7, 15, 16, 1008, 1024, 4095, 16383, 16384])
def test_four_squares(n):
    q = F.four_squares(n)
    assert sum(v * v for v in q) == n and max(q) <= 128 and min(q) >= 0


@pytest.mark.parametrize("fam,D", CELLS)
def test_shapes_and_types(fam, D):
    c = data(fam, D)
    M, T, H = max(dict(F.SHAPES)[D]), F.steps(fam), D // 128
    assert c.xs.shape == (T, M, D) and c.xs.dtype == X.BF and c.W.shape == (3 * D, D) and c.W.dtype == X.BF and c.b.shape == (3 * D,)
    assert c.hist.shape == (M, 2, 3 * D) and c.s0.shape == (M, D, 8) and c.z.shape == (M, T, 3 * D) and c.z.dtype == X.BF and c.H == H
    assert c.ref.y.shape == (M, T, D) and c.ref.states.shape == (M, T, D, 8) and c.ref.hist.shape == (M, T + 2, 3 * D)
    s0r = torch.view_as_real(c.s0)
    assert bool((s0r == s0r.round()).all()) and bool(s0r.any()) and bool(c.hist.any())
    assert torch.equal(torch.view_as_real(c.s0.to(torch.complex64)).double(), s0r)                  # the cast to complex64 is exact
    assert bool((c.g == 1).all())
    small = F.rows(c, 2 if M > 2 else 1)
    again = X.reference(small.z, small.prm, H, z_halo=small.hist, s0=small.s0, check=fam)           # rows are independent
    assert torch.equal(again.y, small.ref.y) and torch.equal(torch.view_as_real(again.states), torch.view_as_real(small.ref.states))


@pytest.mark.parametrize("fam,D", CELLS)
def test_norm_is_exact_in_fp32(fam, D):
    c = data(fam, D)
    x = c.xs.reshape(-1, D)
    assert bool(((x.double() ** 2).sum(-1) == 4096.0 * D).all())
    out, inv = DX.rmsnorm_fp32_emulated(x, c.g)
    assert bool((inv == 2.0 ** -6).all())
    want = x.double() / 64
    assert torch.equal(out.double(), want), int((out.double() != want).sum())
    assert torch.equal(out.to(X.BF).double(), want)                                                 # (the normalised row is a bf16 number)
    src = 2 * want[:, :D - 4]
    assert bool((src == src.round()).all()) and float(src.abs().max()) == 2


@pytest.mark.parametrize("fam,D", CELLS)
def test_projection_is_exact_in_any_order_and_z_is_its_unrounded_result(fam, D):
    c = data(fam, D)
    nz = c.W != 0
    assert int(nz.sum(1).max()) == 1 and bool((c.W[nz].abs() == 2).all()) and not bool(nz[:, D - 4:].any())
    n_zero = int((~nz.any(1)).sum())
    assert n_zero >= D // 16, n_zero                                                                # all-zero rows are there
    n32 = (c.xs.reshape(-1, D).float() / 64)
    z32 = n32 @ c.W.float().t() + c.b.float()                                                       # one non-zero product per sum: any order gives this
    want = c.z.transpose(0, 1).reshape(-1, 3 * D)
    assert torch.equal(z32, want.float()) and torch.equal(z32.to(X.BF).float(), z32)
    if D < 4096:
        flip = n32.flip(-1) @ c.W.float().flip(-1).t() + c.b.float()
        assert torch.equal(flip, z32)
    assert float(c.z.double().abs().max()) <= 3 and bool((c.z.double() == c.z.double().round()).all())
    assert torch.equal(c.ref.hist[:, 2:], c.z.double()) and torch.equal(c.ref.hist[:, :2], c.hist.double())
    if fam == "I":
        x2, x1, v = X._thirds(c.z.double(), c.H)
        assert bool((x1.abs() == v.abs()).all()) and set((x1 * v).unique().tolist()) <= {-4.0, -1.0, 0.0, 1.0, 4.0}
        at = (x1 != 0)
        assert int(at.sum(1).max()) == 1 and not bool(at[:, F.I_IMPULSE_STEPS:].any())             # one impulse per (row, channel), early
        assert 0.3 < float(at.any(1).double().mean()) < 0.7


@pytest.mark.parametrize("fam,D", CELLS)
def test_weight_is_a_fixed_point_of_the_fp8_rule(fam, D):
    c = data(fam, D)
    bytes_, scale = fp8_row_rule(c.W)
    back = Fp8Weight(bytes_, scale).dequantize()
    assert torch.equal(DX.bits(back), DX.bits(c.W))
    zero = (c.W == 0).all(1)
    assert bool(zero.any()) and bool((scale[zero] == 1).all()) and bool((scale[~zero] == 2.0 ** -7).all())


@pytest.mark.parametrize("D,Ms", F.SHAPES)
def test_family_u_share_of_rounded_outputs(D, Ms):
    c = data("U", D)
    for M in Ms:
        share, ties = F.rounded_share(c.ref.y[:M])
        assert share >= 0.1 and ties >= 1, (D, M, share, ties)
    print(f"[hyena_fused_exact host] U D={D}: {100 * share:.1f} % of the outputs are rounded at the store, {ties} exact ties (M = {M})")


@pytest.mark.parametrize("D", [D for D, _ in F.SHAPES])
def test_family_i_impulses_and_poles(D):
    c = data("I", D)
    p = c.prm[2]
    assert bool((p[0::2] != p[1::2]).any(-1).any(-1).all())                                         # the poles of a channel pair differ
    big = c.ref.y.abs() >= X.FLUSH
    tiny = (c.ref.y != 0) & ~big
    assert bool(tiny.any()) and bool(big.any())                                                     # the flush rule has work to do


@pytest.mark.parametrize("fam,D", CELLS)
def test_cpu_replay_of_the_fused_step(fam, D):
    """The oracle's single-token operator on z, from the start state, equals the reference at EVERY step: y, FIR history, modal state."""
    c = data(fam, D)
    fir_w, fir_b, poles, res, dskip = c.prm
    fs, st = c.hist.double().transpose(1, 2), c.s0
    for t in range(c.z.shape[1]):
        y, fs, st = R.op_hyena_step(c.z[:, t], fs, st, fir_w, fir_b, poles, res, dskip, c.H)
        assert torch.equal(y, c.ref.y[:, t]), (t, "y")
        assert torch.equal(fs, X.fir_after(c.ref.hist, t)), (t, "fir")
        assert torch.equal(torch.view_as_real(st), torch.view_as_real(c.ref.states[:, t])), (t, "state")


def _seen(fam, got, ref):
    if got.is_complex():
        got, ref = torch.view_as_real(got.to(torch.complex64)), torch.view_as_real(ref.to(torch.complex64))
    if fam == "U":
        return not bool((got == ref).all())
    a, _ = X.flushed_ok(got, ref)
    b, _ = X.flushed_ok(ref, got)                      # (the kernel, equal to ref, is judged against the MUTANT: that way round too)
    return not bool(a.all()) and not bool(b.all())


@pytest.mark.parametrize("name", F.MUTANTS)
@pytest.mark.parametrize("D,Ms", F.SHAPES)
def test_mutant_table(D, Ms, name):
    """On the very data the GPU module walks, under its rule, at every M: which family sees the mutant, and where."""
    where = {}
    for fam in ("U", "I"):
        c = data(fam, D)
        mut = X.reference(c.z, c.prm, c.H, z_halo=c.hist, s0=c.s0, mutant=name)
        T = c.z.shape[1]
        for M in Ms:
            w = set()
            if _seen(fam, X.round_store(mut.y[:M]), X.round_store(c.ref.y[:M])):
                w.add("y")
            if _seen(fam, mut.states[:M], c.ref.states[:M]):
                w.add("state")
            if any(not torch.equal(X.fir_after(c.ref.hist[:M], t, name), X.fir_after(c.ref.hist[:M], t)) for t in range(T)):
                w.add("fir")
            where[fam, M] = w
    want = {"state_prev_row": ({"y", "state"}, {"y", "state"}), "chan_xor1": ({"y", "state"}, {"y", "state"}),
            "fir_old_kept": ({"y", "state", "fir"}, {"fir"}), "state_early": ({"state"}, {"state"})}[name]
    for M in Ms:
        if name == "state_prev_row" and M == 1:
            assert not where["U", M] and not where["I", M]                                          # (a row mutant needs two rows)
            continue
        assert (where["U", M], where["I", M]) == want, (name, D, M, where["U", M], where["I", M])
        assert (bool(where["U", M]), bool(where["I", M])) == F.CAUGHT[name] and any(F.CAUGHT[name])


@pytest.mark.parametrize("fam,D", CELLS)
def test_swapped_projection_rows_fail_the_fir_rule_at_step_0(fam, D):
    """The rule bites: were the projection rows of two neighbouring channels swapped (here, on the test's side, in W), the z of step 0
    would differ from the reference's, so the GPU module's bit-for-bit check of fir_state fails at step 0."""
    c = data(fam, D)
    zw = c.z[:, 0].double() - c.b.double()                                                          # step 0 without the bias (which stays in place)
    m, j = next((m, j) for m in range(zw.shape[0]) for j in range(0, 3 * D, 2) if zw[m, j] != zw[m, j + 1])
    Wsw = c.W.clone()
    Wsw[[j, j + 1]] = c.W[[j + 1, j]]
    zsw = ((c.xs[0, m:m + 1].double() / 64) @ Wsw.double().t() + c.b.double()).to(X.BF)             # [1, 3 D]: step 0, row m
    assert torch.equal(zsw[:, :j], c.z[m:m + 1, 0, :j]) and torch.equal(zsw[:, j + 2:], c.z[m:m + 1, 0, j + 2:])
    hist = c.ref.hist[m:m + 1, :3].clone()
    want = X.fir_after(hist, 0).to(X.BF)
    hist[:, 2] = zsw.double()
    got = X.fir_after(hist, 0).to(X.BF)
    assert int((DX.bits(got) != DX.bits(want)).sum()) == 2
    print(f"[hyena_fused_exact host] {fam} D={D}: projection rows {j}, {j + 1} swapped -> fir_state of row {m} differs at step 0")
