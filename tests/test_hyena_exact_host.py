"""CPU: the exact Hyena designs of tests/hyena_exact.py are pinned to the OPERATION (the project's fp64 oracle op), the CPU emulation of
csrc/hyena_ct.hip's operand precisions (tests/test_hyena_blocked.py: emulate_blocked) reproduces the per-step reference bit for bit before
the output rounding, the generators' exactness conditions hold for every case the GPU module uses, and every deliberately wrong reference
differs from the true one after the bf16 rounding -- the defects tests/test_gpu_hyena_exact.py is there to catch.

Which family sees which mutant (asserted below, `CAUGHT`):
    mutant               U     I
    fir_reversed         yes   yes    (I: the identity FIR moves by two steps)
    tile_hist_zero       yes   no     (I's FIR reads no history)
    row_hist_prev_row    yes   no     (the same)
    swap_reim            yes   yes
    carry_block_off      yes   yes
    pow_plus4            NO    yes    (p^4 = 1 on U's poles: the reason family I exists)
    mode_xor1            yes   yes
    state_early          yes   yes    (the end state; y is untouched)
    trunc_store          yes   yes    (I: only through s0's response, up to 9 significant bits; an impulse's own has <= 4: no rounding)
    state_prev_row       yes   yes    (the single-token launches' defects, tests/hyena_fused_exact.py: here through the rows' start states)
    chan_xor1            yes   yes
    fir_old_kept         yes   no     (I's FIR reads no history; the fused launches' walks see it in fir_state)
"""
import pytest
import torch

import hyena_exact as X
from oracle import stripedhyena_ref as R
from test_hyena_blocked import emulate_blocked

CAUGHT = X.CAUGHT
TINY_POLE = 2.0 ** -200     # the oracle's exp(t log p) has no value at p = 0 (family I): it is handed this instead; |difference| < 2^-190


def _oracle(z, prm, H, **kw):
    fir_w, fir_b, poles, res, dskip = prm
    poles = poles.double().clone()
    zero = (poles == 0).all(-1)
    poles[..., 0] = torch.where(zero, torch.full_like(poles[..., 0], TINY_POLE), poles[..., 0])
    return R.op_hyena(z, fir_w, fir_b, poles, res, dskip, H, **kw)


# ------------------------------------------------------------------------------------------------ the reference computes the operation
@pytest.mark.parametrize("variant", ["plain", "halo_s0", "mask"])
@pytest.mark.parametrize("fam,B,T,D,H", [("U", 2, 37, 128, 1), ("U", 1, 700, 256, 2), ("I", 2, 700, 256, 2)])
def test_reference_is_the_oracles_function(fam, B, T, D, H, variant):
    """1e-8 max|ref|: the oracle (FFT convolution, exp(t log p)) is the inexact one here; this pins only that both compute the same
    function -- the thirds of a head, the FIR taps' order, the halo rows, the start state, the padding mask."""
    hs = variant == "halo_s0"
    z, prm, halo, s0, ref = X.make(fam, B, T, D, H, 3, halo=hs, s0=hs)
    kw = dict(z_halo=halo, s0=s0) if hs else {}
    if variant == "mask":
        mask = torch.ones(B, T, dtype=torch.bool)
        mask[0, 0] = False
        mask[0, T // 3:T // 3 + 5] = False
        mask[-1, T - 7:] = False
        kw = dict(mask=mask)
        ref = X.reference(z, prm, H, mask=mask)
    ry, rst = _oracle(z, prm, H, **kw)
    assert float((ref.y - ry).abs().max()) <= 1e-8 * float(ry.abs().max())
    assert float((ref.states[:, -1] - rst).abs().max()) <= 1e-8 * float(rst.abs().max())
    assert torch.equal(ref.hist[:, 2:], z.double()) and (halo is None or torch.equal(ref.hist[:, :2], halo.double()))


def test_reference_prefix_property():
    """The state at step t of a long run is the end state of a run of t + 1 steps, and y likewise: bit for bit."""
    for fam in ("U", "I"):
        z, prm, halo, s0, ref = X.make(fam, 2, 600, 128, 1, 5, halo=True, s0=True)
        for t in (0, 1, 31, 32, 511, 512, 598):
            short = X.reference(z[:, :t + 1], prm, 1, halo, s0)
            assert torch.equal(torch.view_as_real(short.states[:, -1]), torch.view_as_real(ref.states[:, t])), (fam, t)
            assert torch.equal(short.y, ref.y[:, :t + 1]) and torch.equal(short.hist, ref.hist[:, :t + 3])
        at = torch.tensor([[0, 511], [598, 32]])
        some = X.reference(z, prm, 1, halo, s0, state_at=at)
        for b in range(2):
            assert torch.equal(torch.view_as_real(some.states[b]), torch.view_as_real(ref.states[b, at[b]]))


# ------------------------------------------------------------------------------------------------ the kernel's operand precisions hold it exactly
@pytest.mark.parametrize("fam", ["U", "I"])
@pytest.mark.parametrize("B,T,D", [(2, 37, 128), (1, 1100, 128), (1, 2600, 128), (1, 8 * 512 + 8, 128)])
def test_blocked_emulation_is_bit_exact(fam, B, T, D):
    """emulate_blocked (bf16 hi / lo data and tables, fp32 accumulation and scan, bf16-split states) == the reference BEFORE the output
    rounding: 0 differing elements (family I: in its exact region; |emulation| <= 2^-99 in the flushed tails)."""
    z, prm, _, _, ref = X.make(fam, B, T, D, 1, 9)
    out, _ = emulate_blocked(z, *prm, 1)
    if fam == "U":
        assert torch.equal(out.double(), ref.y)
        need = float((ref.y.to(X.BF).double() != ref.y).double().mean())
        assert need > 0.25 or T < 1000, need                              # a good share of the outputs needs a non-trivial rounding
        print(f"[hyena exact] U {B} x {T} x {D}: max |state| {float(torch.view_as_real(ref.states).abs().max()):.0f}, max |y| "
              f"{float(ref.y.abs().max()):.0f}, {100 * need:.1f} % of the outputs are rounded at the store")
    else:
        ok, n_tiny = X.equal_or_flushed(out, ref.y.float())
        assert bool(ok.all()), int((~ok).sum())
        nz = int((ref.y != 0).sum())
        print(f"[hyena exact] I {B} x {T} x {D}: {n_tiny} of {nz} non-zero reference elements under the flush rule ({100.0 * n_tiny / max(1, nz):.1f} %)")


# ------------------------------------------------------------------------------------------------ the generators' conditions, every GPU case
@pytest.mark.parametrize("fam", ["U", "I"])
def test_generator_conditions_hold_for_every_gpu_case(fam):
    """family_u / family_i assert their exactness conditions on the reference; this runs them for every (shape, seed) of the GPU module."""
    cases = [c for c in X.gpu_cases() if c[0] == fam]
    assert len(cases) > 20 and len(X.gpu_cases()) == len([c for c in X.gpu_cases() if c[0] in ("U", "I")])
    for _, B, T, D, H, seed, halo, s0, state_at in cases:
        z, prm, zh, s_in, ref = X.make(fam, B, T, D, H, seed, halo=halo, s0=s0, state_at=state_at)
        assert z.shape == (B, T, 3 * D) and ref.y.shape == (B, T, D) and (zh is not None) == halo and (s_in is not None) == s0


def test_state_at_lens_cover_every_length():
    for B, T, _, _ in X.STATE_AT:
        lens = X.state_at_lens(B, T)
        assert lens.shape[1] == B and sorted(set(lens.reshape(-1).tolist())) == list(range(1, T + 1))


# ------------------------------------------------------------------------------------------------ the mutants
@pytest.fixture(scope="module")
def mutant_data():
    out = {}
    for fam in ("U", "I"):
        S = X.SWEEP                                                       # the GPU module holds the kernels against the same mutants on this data
        out[fam] = X.make(fam, S["B"], S["T"], S["D"], S["H"], S["seed"], halo=True, s0=True)
    return out


@pytest.mark.parametrize("name,what", X.mutants())
def test_every_mutant_is_caught(mutant_data, name, what):
    """After the bf16 rounding (y) / the complex64 cast (end state) a mutant differs from the true reference exactly on the families of
    CAUGHT -- at least one each; p^(k + 4) is invisible to U and caught by I."""
    seen = []
    for fam in ("U", "I"):
        z, prm, halo, s0, ref = mutant_data[fam]
        if name == "trunc_store":
            differs = not torch.equal(X.round_store(ref.y, name).view(torch.int16), X.round_store(ref.y).view(torch.int16))
        else:
            mut = X.reference(z, prm, 1, halo, s0, mutant=name)
            if what == "y":
                ok, _ = X.equal_or_flushed(X.round_store(mut.y), X.round_store(ref.y))
            else:
                assert torch.equal(mut.y, ref.y)
                ok, _ = X.equal_or_flushed(torch.view_as_real(mut.states[:, -1].to(torch.complex64)),
                                           torch.view_as_real(ref.states[:, -1].to(torch.complex64)))
            differs = not bool(ok.all())
        seen.append(differs)
    assert tuple(seen) == CAUGHT[name], (name, seen)
    assert any(seen)


def test_mutant_table_is_complete():
    assert sorted(CAUGHT) == sorted(n for n, _ in X.mutants()) and all(any(v) for v in CAUGHT.values())
    assert CAUGHT["pow_plus4"] == (False, True)
