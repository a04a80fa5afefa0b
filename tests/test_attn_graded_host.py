"""CPU: design G of tests/attn_exact.py (graded softmax weights: every weight an exact power of two) is pinned to the OPERATION (the
project's fp64 oracle op), its exactness conditions are recomputed in int64, plain-torch emulations of the w64 bookkeeping and of the
stream split + combine reproduce every case under the rule, and the judge is shown to fail on wrong ARITHMETIC -- skipped small weights,
a wrong or half-applied rescale factor, a wrong combine weight, a dropped light key, a neighbour's mu -- that the tolerance tests' pin
|err| <= 2^-8 |ref| + 2e-2 lets through (the count it would flag is printed beside each).  tests/test_gpu_attn_graded.py uses the
same lists on the kernels.

A defect is judged at every case of the lists: it must FAIL wherever it changes the emulation's output at all; where the output is
bit-identical the defect is unreachable on that case (a flat PRE row never moves its reference point: alpha is 1 throughout), and each
test asserts the set of cases on which its defect must be reachable."""

import numpy as np
import pytest
import torch

import attn_exact as X
from oracle_ops import OracleOps

BF = torch.bfloat16
FORMS = [(True, None), (False, 1.0)]                                    # PRE; plain at softmax_scale = G_LN2 (c = 1)
PREFILL = [s for s, _, _ in X.G_W64[:5]] + X.G_QB128                    # every distinct prefill shape of the GPU lists (G_PIPE is a subset)
W_DEFECTS = ["skip8", "skip12", "alpha_err", "alpha_l_only", "alpha_o_only"]


def _prefill_case(shape, stair, B=1, H=1, P=0):
    return X.graded_prefill(shape, B, H, X.DIMS2[1], stair, P=P)


def _ref(c, n_splits=0):
    return X.expected_graded(c["e"], c["mu"], c["v"], c["mult"]), X.graded_allow(c["mult"], c["stair"], n_splits)


# ------------------------------------------------------------------------------------------------ the plain form's scale
def test_ln2_scale_makes_scale_log2_one():
    """softmax_scale = G_LN2 is an fp32 number and the entries' own `softmax_scale * 1.4426950408889634f` is 1.0f exactly."""
    s = np.float32(X.G_LN2)
    assert float(s) == X.G_LN2
    assert s * np.float32(1.4426950408889634) == np.float32(1.0)
    assert (torch.tensor(X.G_LN2, dtype=torch.float32) * torch.tensor(1.4426950408889634, dtype=torch.float32)).item() == 1.0


# ------------------------------------------------------------------------------------------------ exactness, in integers
def _all_cases():
    """(name, case, n_splits) for every case of the GPU lists, with the lists' batch sizes at H = 1 (a head only scales V by a power of
    two: the conditions do not depend on it)."""
    out = []
    for stair in X.G_VARIANTS:
        for shape, B in sorted({(s, b) for s, b, _ in X.G_W64} | {(s, 3) for s in X.G_QB128 + X.G_PIPE}):
            out.append((f"prefill {shape} B {B} {stair}", _prefill_case(shape, stair, B=B), 0))
        for P, Tq in X.G_PREFIX:
            out.append((f"prefix P {P} Tq {Tq} {stair}", _prefill_case((Tq, P, 0), stair, B=3, P=P), 0))
        out.append((f"decode {stair}", X.graded_decode(X.G_DECODE_STAIR, 1, X.DIMS2[0], stair), 40))
    out.append((f"prefill {X.G_QB128_LONG} flat", _prefill_case(X.G_QB128_LONG, None, B=3), 0))
    out.append(("decode long flat", X.graded_decode(X.DECODE_POSITIONS, 1, X.DIMS2[0], None), 40))
    return out


def test_integer_sums_fit_24_bits():
    """Flat cases: with every weight scaled to an integer (2^(mu e - the row's smallest exponent)) a row's whole sum stays below 2^24, so
    every partial sum of l and of any output dim is an fp32 integer times a power of two.  Stair cases: the same inside every 64-key tile
    for the levels that meet there within 3 units; every other pair of levels in one tile is >= 30 apart (graded_check)."""
    for name, c, _ in _all_cases():
        for b in range(c["e"].shape[0]):
            ex = c["mu"][b][:, None] * c["e"][b][None, :]
            vis = c["mult"][b] > 0
            if c["stair"] is None:
                lo = torch.where(vis, ex, torch.full_like(ex, 1 << 40)).min(-1, keepdim=True).values
                tot = torch.where(vis, torch.ones_like(ex) << (ex - lo).clamp(0, 40), torch.zeros_like(ex)).sum(-1)
                assert int(tot.max()) < 1 << 24, name
            else:
                hi = torch.where(vis, ex, torch.full_like(ex, -(1 << 40))).max(-1).values
                lo = torch.where(vis, ex, torch.full_like(ex, 1 << 40)).min(-1).values
                assert int((hi - lo).max()) <= X.G_SPAN, name                               # per row: nothing leaves the normal range


def test_builder_refuses_what_is_not_exact():
    with pytest.raises(AssertionError):
        X.graded_check(2050, 7, X.G_MUS)                                # 12 + 14 bits
    with pytest.raises(AssertionError):
        X.graded_check(8229, 6, X.G_MUS)                                # 14 + 12 bits
    with pytest.raises(AssertionError):
        X.graded_check(642, 4, (1, -1, 1), "W1")                        # a twelfth block
    X.graded_check(8229, 5, X.G_MUS)
    X.graded_check(2049, 6, X.G_MUS)
    for stair, (lv, mus) in X.G_STAIRS.items():
        X.graded_check(641, X.G_WIN_STAIR, mus, stair)
        X.graded_check(641, X.G_WIN_STAIR, mus, stair, X.graded_cuts(320))
        steps = {lv[n + 1] - lv[n] for n in range(len(lv) - 1)}
        assert steps & {31, 32, 33, 63, 64, 65, -40, -70, 65} or lv[0] == -65


# ------------------------------------------------------------------------------------------------ the reference vs the oracle op
@pytest.mark.parametrize("stair", X.G_VARIANTS)
def test_expected_graded_is_the_fp64_softmax(stair):
    """expected_graded == OracleOps.attention on the same bf16 inputs to 1e-12 (the scores are log2 exponents: q / c gives the oracle's
    exp(q.k / sqrt(128)) the same softmax), prefill and decode."""
    c = X.graded_prefill((150, 63, 0), 2, 2, X.DIMS2[2], stair)
    ref, _ = _ref(c)
    want = OracleOps().attention(c["q"].double() / X.C_LOG2, c["k"], c["v"], 63)
    assert bool(((ref - want).abs() <= 1e-12 * want.abs()).all())
    pos = [0, 1, 63, 64, 65, 200, 555]
    c = X.graded_decode(pos, 2, X.DIMS2[0], stair)
    ref, _ = _ref(c)
    want = OracleOps().attention_decode(c["q"].double() / X.C_LOG2, c["k"], c["v"], torch.tensor(pos))
    assert bool(((ref - want).abs() <= 1e-12 * want.abs()).all())


def test_allowance_zone_share_is_under_the_cap():
    """A condition on the INPUTS, from the fp64 reference alone: in every case of the lists fewer than 0.1 % of the elements lie inside
    their allowance zone, so the cap cannot be what lets a case pass."""
    worst = 0.0
    for name, c, ns in _all_cases():
        ref, allow = _ref(c, ns)
        share = X.zone_share(ref, allow)
        worst = max(worst, share)
        assert share < X.ALLOW_SHARE, f"{name}: {100 * share:.4f} % of the elements lie in the allowance zone"
        nz = ref[ref != 0].abs()
        assert float(nz.min()) >= 2.0 ** -126 and float(nz.max()) < 2.0 ** 4, name          # normal bf16 numbers
    print(f"[attn graded] largest allowance-zone share over {len(_all_cases())} cases: {100 * worst:.4f} %")


# ------------------------------------------------------------------------------------------------ the emulations under the rule
def _emu_w64(c, q_pos0, pre, cc, defect=None):
    return torch.stack([X.emulate_w64(c["q"][b, :, 0], c["k"][b, :, 0], c["v"][b, :, 0], q_pos0, pre, cc, defect)
                        for b in range(c["q"].shape[0])])[:, :, None]


@pytest.mark.parametrize("stair", X.G_VARIANTS, ids=str)
def test_w64_emulation_reproduces_every_prefill_case(stair):
    """PRE (W_THRP, the reference at 0) and plain at c = 1 (W_THR, the first tile's maximum as the reference): 0 elements outside the
    rule; flat cases do not use the allowance at all."""
    for shape in PREFILL + ([X.G_QB128_LONG] if stair is None else []):
        c = _prefill_case(shape, stair)
        ref, allow = _ref(c)
        for pre, cc in FORMS:
            ver = X.judge_graded(_emu_w64(c, shape[1], pre, cc), ref, allow)
            assert ver.ok and (stair is not None or ver.n_allowed == 0), f"{shape} {stair} {'PRE' if pre else 'c = 1'}: {ver}"


def test_w64_emulation_existing_callers_unchanged():
    """The optional arguments change nothing for the callers of before: c = None is C_LOG2, bit for bit."""
    c = X.build_case("S", 1, 1, 200, 5, 205, X.DIMS2[0])
    for pre in (False, True):
        a = X.emulate_w64(c["q"][0, :, 0], c["k"][0, :, 0], c["v"][0, :, 0], 5, pre)
        b = X.emulate_w64(c["q"][0, :, 0], c["k"][0, :, 0], c["v"][0, :, 0], 5, pre, X.C_LOG2, None)
        assert torch.equal(a.view(torch.int16), b.view(torch.int16))


def _emu_stream(c, positions, ns, defect=None):
    outs = [X.emulate_stream(c["q"][b, 0, 0], c["k"][b, :p + 1, 0], c["v"][b, :p + 1, 0], ns, 1.0, defect) for b, p in enumerate(positions)]
    return torch.stack([o for o, _, _ in outs])[:, None, None], torch.stack([po for _, po, _ in outs]), torch.stack([ml for _, _, ml in outs])


def _decode_cases():
    return [(X.DECODE_POSITIONS, None)] + [(X.G_DECODE_STAIR, s) for s in X.G_VARIANTS]


@pytest.mark.parametrize("ns", [1, 4, 8, 40, 32])
def test_stream_emulation_reproduces_every_decode_case(ns):
    """The split + combine emulation: 0 elements outside the rule; on the flat case its fp32 partials ARE the closed forms."""
    for positions, stair in _decode_cases():
        c = X.graded_decode(positions, 1, X.DIMS2[0], stair)
        ref, allow = _ref(c, ns)
        got, po, ml = _emu_stream(c, positions, ns)
        ver = X.judge_graded(got, ref, allow)
        assert ver.ok and (stair is not None or ver.n_allowed == 0), f"decode {stair} n_splits {ns}: {ver}"
        if stair is None:
            want_o, want_ml = X.stream_partials_expected(c, positions, ns)
            assert torch.equal(ml.view(torch.int32), want_ml[:, 0].view(torch.int32))
            assert torch.equal(po.view(torch.int32), want_o[:, 0].view(torch.int32))


# ------------------------------------------------------------------------------------------------ wrong arithmetic must fail
def _verdict_of_defect(name, got, clean, ref, allow, must):
    """-> 'unreachable' | 'fails'; asserts that a reachable defect fails and that `must` cases are reachable."""
    if torch.equal(got.view(torch.int16), clean.view(torch.int16)):
        assert not must, f"{name}: the defect does not change the output"
        return "unreachable", 0
    ver = X.judge_graded(got, ref, allow)
    assert not ver.ok and ver.n_bad > 0, f"{name}: the judge passes a wrong arithmetic: {ver}"
    return "fails", X.old_pin_count(got, ref)


@pytest.mark.parametrize("defect", W_DEFECTS)
def test_w64_defects_fail(defect):
    """attn_fwd_w64_kernel's arithmetic with one thing wrong, at every prefill case and both forms.  Must be reachable: skip8 on every
    flat case with a row of mu = 2 (2 win > 8), skip12 on the flat cases up to 1,023 keys (2 * 7 = 14 > 12), alpha_err on every flat case of
    two tiles or more, the half-applied alpha on every stair case of more than 320 keys and three rows (by then a row of every list has
    moved a reference point with something accumulated, in both forms)."""
    seen = {"fails": 0, "unreachable": 0}
    old = 0
    for stair in X.G_VARIANTS:
        for shape in PREFILL:
            Tq, q_pos0, dTk = shape
            c = _prefill_case(shape, stair)
            ref, allow = _ref(c)
            for pre, cc in FORMS:
                clean = _emu_w64(c, q_pos0, pre, cc)
                got = _emu_w64(c, q_pos0, pre, cc, defect)
                if defect == "skip8":
                    must = stair is None and Tq >= 3
                elif defect == "skip12":
                    must = stair is None and Tq >= 3
                elif defect == "alpha_err":
                    must = stair is None and q_pos0 + Tq + dTk > 64          # (a stair row may end on a level that outweighs all before it)
                else:
                    must = stair is not None and q_pos0 + Tq + dTk > 320 and Tq >= 3
                r, n = _verdict_of_defect(f"{defect} {shape} {stair} {'PRE' if pre else 'c = 1'}", got, clean, ref, allow, must)
                seen[r] += 1
                old += n
    print(f"[attn graded] w64 {defect}: fails at {seen['fails']} cases, unreachable at {seen['unreachable']}; the pin 2^-8 |ref| + 2e-2 "
          f"would flag {old} elements in all")
    assert seen["fails"] >= 10


@pytest.mark.parametrize("defect", W_DEFECTS + ["combine_m_next", "tail_unweighted"])
def test_stream_defects_fail(defect):
    """The stream split + combine with one thing wrong, at every decode case and split count.  The combine defects must be reachable
    on the stair cases at 4 and 8 splits (their splits end on different maxima; below 29 splits the whole combine is its tail loop).  At
    40 splits the tail loop takes splits 32 .. 39: on the long flat case they all hold keys but share one maximum with the rest, on the
    short cases they are empty -- the tail loop's weighting is pinned by the cases below 29 splits, which run the same statement."""
    seen = {"fails": 0, "unreachable": 0}
    old = 0
    for ns in (1, 4, 8, 40, 32):
        for positions, stair in _decode_cases():
            c = X.graded_decode(positions, 1, X.DIMS2[0], stair)
            ref, allow = _ref(c, ns)
            clean, _, _ = _emu_stream(c, positions, ns)
            got, _, _ = _emu_stream(c, positions, ns, defect)
            if defect in ("combine_m_next", "tail_unweighted"):
                must = stair is not None and ns in (4, 8)
            elif defect in ("alpha_l_only", "alpha_o_only"):
                must = stair is not None and ns in (1, 4)
            elif defect == "alpha_err":
                must = ns == 1
            elif defect == "skip8":
                must = stair is None
            else:
                must = stair is None and positions is X.G_DECODE_STAIR               # win = 7 up to 1,023 keys
            r, n = _verdict_of_defect(f"{defect} decode {stair} n_splits {ns}", got, clean, ref, allow, must)
            seen[r] += 1
            old += n
    print(f"[attn graded] stream {defect}: fails at {seen['fails']} cases, unreachable at {seen['unreachable']}; the pin 2^-8 |ref| + 2e-2 "
          f"would flag {old} elements in all")
    assert seen["fails"] >= 3


def _light_keys_at_seams(c, q_pos0):
    """One key of weight 2^-win (g = win) per seam: the nearest such key at or behind each of prefill_seams / the cuts."""
    Tk = c["e"].shape[1]
    seams = sorted(set(X.prefill_seams(c["mult"].shape[1], q_pos0, Tk)) | {t for t in X.G_CUTS if t < Tk})
    lv = X.graded_exponents(1, Tk, 0, c["stair"])[0]                    # win = 0: the bare levels
    out = []
    for b in range(c["e"].shape[0]):
        light = (lv - c["e"][b] == c["win"]).nonzero().flatten()
        out.append(sorted({int(light[light >= t][0]) for t in seams if bool((light >= t).any())}))
    return out


@pytest.mark.parametrize("stair", X.G_VARIANTS, ids=str)
def test_a_dropped_light_key_fails(stair):
    """One key of the SMALLEST weight (2^-win under mu = 1) lost at each seam: what a row returns then is expected_graded on the edited
    multiplicities; the judge fails it at every prefill case (on the rows where that key is not 30 levels down)."""
    old = 0
    for shape in PREFILL:
        Tq, q_pos0, dTk = shape
        c = _prefill_case(shape, stair)
        ref, allow = _ref(c)
        mult = c["mult"].clone()
        for b, ts in enumerate(_light_keys_at_seams(c, q_pos0)):
            mult[b][:, ts] = 0
        if bool((mult.sum(-1) == 0).any()) or torch.equal(mult, c["mult"]):
            continue                                                    # (a row whose only key it was: the one-row case)
        got = X.expected_graded(c["e"], c["mu"], c["v"], mult).to(BF)
        ver = X.judge_graded(got, ref, allow)
        assert not ver.ok and ver.n_bad > 0, f"{shape} {stair}: {ver}"
        old += X.old_pin_count(got, ref)
    print(f"[attn graded] dropped light keys {stair}: the pin 2^-8 |ref| + 2e-2 would flag {old} elements in all")


@pytest.mark.parametrize("shift", [1, -1])
@pytest.mark.parametrize("stair", X.G_VARIANTS, ids=str)
def test_a_neighbours_mu_fails(stair, shift):
    """Row i computed with row i +- 1's query (mu of the neighbour): every prefill case of more than one row, and decode by batch row."""
    for shape in [s for s in PREFILL if s[0] > 1]:
        c = _prefill_case(shape, stair)
        ref, allow = _ref(c)
        got = X.expected_graded(c["e"], torch.roll(c["mu"], shift, 1), c["v"], c["mult"]).to(BF)
        ver = X.judge_graded(got, ref, allow)
        assert not ver.ok and int(ver.bad.sum()) >= shape[0] // 3, f"{shape} {stair}: {ver}"
    positions = X.DECODE_POSITIONS if stair is None else X.G_DECODE_STAIR
    c = X.graded_decode(positions, 1, X.DIMS2[0], stair)
    ref, allow = _ref(c, 4)
    got = X.expected_graded(c["e"], torch.roll(c["mu"], shift, 0), c["v"], c["mult"]).to(BF)
    assert not X.judge_graded(got, ref, allow).ok


# ------------------------------------------------------------------------------------------------ what the design cannot see
def test_truncated_p_passes():
    """P packed to bf16 by TRUNCATION instead of rounding: every weight of G is a power of two, a bf16 number either way -- the outputs
    are bit-identical and the judge passes.  The rounding of P stays with the tolerance tests (PARITY row 12b says so)."""
    for stair in X.G_VARIANTS:
        c = _prefill_case((321, 63, 0), stair)
        ref, allow = _ref(c)
        for pre, cc in FORMS:
            clean = _emu_w64(c, 63, pre, cc)
            got = _emu_w64(c, 63, pre, cc, "trunc_p")
            assert torch.equal(got.view(torch.int16), clean.view(torch.int16)) and X.judge_graded(got, ref, allow).ok
    r = X.build_case("U", 1, 1, 200, 0, 200, X.DIMS2[0])               # (the defect is real: on non-dyadic weights it changes bits)
    q = (torch.randn(200, 128, generator=torch.Generator().manual_seed(1)) * 3).to(BF)
    a = X.emulate_w64(q, r["k"][0, :, 0], r["v"][0, :, 0], 0, True)
    b = X.emulate_w64(q, r["k"][0, :, 0], r["v"][0, :, 0], 0, True, None, "trunc_p")
    assert not torch.equal(a.view(torch.int16), b.view(torch.int16))
