"""CPU: the exact attention designs of tests/attn_exact.py are pinned to the OPERATION (the project's fp64 oracle op), their arithmetic
claims are recomputed in int64 / fp64, a plain-torch emulation of the w64 bookkeeping reproduces them bit for bit, and the judge is shown
to fail on every row of a wrong key set -- the defects tests/test_gpu_attn_exact.py is there to catch."""
import pytest
import torch

import attn_exact as X
from oracle_ops import OracleOps

BF = torch.bfloat16
SMALL = [(70, 0, 0), (70, 5, 12), (40, 130, -9)]            # (Tq, q_pos0, Tk - (q_pos0 + Tq)): diagonal, canaries inside Tk, ragged end


def _case(design, shape, B=2, H=2, dims=X.DIMS2[1]):
    Tq, q_pos0, dTk = shape
    return X.build_case(design, B, H, Tq, q_pos0, q_pos0 + Tq + dTk, dims), q_pos0


def _close(a, b):
    return bool(((a - b).abs() <= 1e-12 * b.abs()).all())


# ------------------------------------------------------------------------------------------------ closed forms vs the oracle op
@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("shape", SMALL)
@pytest.mark.parametrize("design", X.DESIGNS)
def test_closed_forms_are_the_fp64_softmax(design, shape, pre):
    """mean over the visible set / V[last] / V[0] / V[t_m] == OracleOps.attention of the same bf16 inputs to 1e-12, plain form with its
    real scale (the oracle's 1 / sqrt(128)) and PRE (the scores are log2 exponents: q / c gives the oracle the same softmax)."""
    c, q_pos0 = _case(design, shape)
    ref, single = X.expected(c["lev"], c["v"], c["mult"])
    q = c["q"].double() / X.C_LOG2 if pre else c["q"]
    want = OracleOps().attention(q, c["k"], c["v"], q_pos0)
    assert _close(ref, want)
    assert bool(single.all()) == (design in ("D", "D'"))
    if design == "S":
        assert bool((~single).any()) and bool(single.any())          # both the U mean in front of t_1 and V[t_m] rows occur


@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("design", X.DESIGNS)
def test_decode_closed_forms_are_the_fp64_softmax(design, pre):
    pos = [0, 1, 63, 64, 65, 200]
    c = X.build_decode(design, pos, 2, X.DIMS2[0], 4)
    ref, _ = X.expected(c["lev"], c["v"], c["mult"])
    q = c["q"].double() / X.C_LOG2 if pre else c["q"]
    want = OracleOps().attention_decode(q, c["k"], c["v"], torch.tensor(pos))
    assert _close(ref, want)


# ------------------------------------------------------------------------------------------------ the w64 bookkeeping, emulated
@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("design", X.DESIGNS)
def test_w64_emulation_is_bit_exact(design, pre):
    """64-key tiles, deferred reference point (0 inside +-W_THRP in PRE, moved to the tile maximum beyond), P rounded to bf16, l from the
    unrounded weights: D, D', S rows come out as the V row's pattern, U rows as bf16(count / n) without any use of the allowance."""
    c, q_pos0 = _case(design, (321, 63, 0), B=1, H=1)
    ref, single = X.expected(c["lev"], c["v"], c["mult"])
    got = X.emulate_w64(c["q"][0, :, 0], c["k"][0, :, 0], c["v"][0, :, 0], q_pos0, pre)[None, :, None]
    ver = X.judge(got, ref, single)
    assert ver.n_bad == 0 and ver.n_allowed == 0, ver
    rows = single[0]
    assert torch.equal(got[0, rows].view(torch.int16), ref[0, rows].to(BF).view(torch.int16))


# ------------------------------------------------------------------------------------------------ the values
def test_v_id_is_finite_normal_and_distinct():
    v = X.v_id(3, 2049, 2)
    pat = v.view(torch.int16).to(torch.int64) & 0xffff
    ex, man = (pat >> 7) & 0xff, pat & 0x7f
    assert int(ex.min()) == 97 and int(ex.max()) == 157                 # 2^-30 .. 2^30: no subnormal, no zero, no inf / NaN
    assert set(man.unique().tolist()) == set(range(128)) and set((pat >> 15).unique().tolist()) == {0, 1}
    assert torch.isfinite(v.float()).all()
    assert X.min_distinct_dims(v) >= 100
    assert not torch.equal(v[0], v[1]) and not torch.equal(v[:, :, 0], v[:, :, 1])


@pytest.mark.parametrize("B,H,T", [(1, 8, 578), (12, 2, 200), (2, 2, 2100)])
def test_v_id_distinct_for_the_gpu_shapes(B, H, T):
    """>= 100 of 128 dims differ by more than one bf16 ulp for every |j - j'| <= 64: the (B, H) pairs of the GPU module at their longest
    key ranges (a value depends on (b, h, key, dim) only, so a shorter range is a block of these)."""
    assert X.min_distinct_dims(X.v_id(B, T, H)) >= 100


def test_v_id_distinct_for_the_long_decode_rows():
    for b, p in zip((10, 11), (2080, 8228)):                           # the two long rows of the mixed decode batch, their own keys
        assert X.min_distinct_dims(X.v_id(b + 1, p + 1, 2)[b:]) >= 100


def test_v_hist_counts_are_exact_and_v_alt_prefix_sums_stay_in_01():
    T = X.HIST_MAX_KEYS
    v = X.v_hist(1, T, 1)[0, :, 0]
    cs64, cs32 = v.double().cumsum(0), v.float().cumsum(0)
    assert torch.equal(cs64, cs32.double())                            # every prefix sum exact in fp32
    s = float(X.head_factor(1, 1).reshape(()))
    assert float(cs64.max()) == 65 * s and float(cs64[-1].sum()) == T * s
    a = X.v_hist(1, 4096, 1, alt=True)[0, :, 0].double().cumsum(0) / s
    assert set(a.unique().tolist()) == {0.0, 1.0}
    # one aligned run of 256 keys sums to zero in every class: V_alt cannot see it go missing (V_hist does)
    assert float(X.v_hist(1, 4096, 1, alt=True)[0, 512:768, 0].double().sum(0).abs().max()) == 0.0


def test_one_key_moves_a_v_hist_output_by_ulps():
    """Dropping the last key of a row of n keys changes its class from k / n to (k - 1) / (n - 1), counting it twice to (k + 1) / (n + 1).
    In units of the bf16 spacing at k / n (2^-8 of the binade's lower end): 123 at 64 keys, 7.4 at 2,049, 1.9 at 8,229 -- each side rounds
    by at most half a spacing, so more than one spacing apart is a different pattern at every length V_hist is used for."""
    for n, least in ((64, 123.0), (2049, 7.4), (8229, 1.9)):
        k = (n - 1) // 128 + 1
        a = torch.tensor(k / n, dtype=torch.float64)
        ulp = 2.0 ** (torch.frexp(a)[1].item() - 8)
        moved = min(abs(k / n - (k - 1) / (n - 1)), abs(k / n - (k + 1) / (n + 1))) / ulp
        assert moved >= least and moved > 1.0, (n, moved)


def _u_cases():
    for Tq, q_pos0, dTk in X.W64_SHAPES + X.QB128_SHAPES:
        yield X.causal_mult(1, Tq, q_pos0 + Tq + dTk, q_pos0), q_pos0 + Tq + dTk
    for P, Tq in X.PREFIX_SHAPES:
        yield X.causal_mult(1, Tq, P + Tq, P), P + Tq
    for p in X.DECODE_POSITIONS + X.MFMA_POSITIONS:
        yield X.decode_mult([p], p + 1), p + 1


def test_boundary_allowance_cap_holds_for_every_gpu_shape():
    """At most 0.1 % of a U case's elements lie within 2^-21 |ref| of a bf16 rounding boundary (s_bh is a power of two: the share does
    not depend on the batch row or head), and the kernels' two-rounding form fp32(S) * fp32(1 / n) gives bf16(fp64) everywhere else."""
    worst = 0.0
    for mult, Tk in _u_cases():
        v = X.v_hist(1, Tk, 1)
        ref, _ = X.expected(torch.zeros(1, Tk, dtype=torch.int64), v, mult)
        e, _, dist = X.bf16_neighbourhood(ref)
        near = (dist <= X.ALLOW_REL * ref.abs()) & (ref != 0)
        worst = max(worst, float(near.sum()) / ref.numel())
        n = mult.sum(-1).float()
        two = ((mult.float() @ v[0, :, 0].float()) * (1.0 / n)[..., None]).to(BF).double()[:, :, None]
        assert bool(((two == e) | near).all())
    assert worst <= X.ALLOW_SHARE, worst


# ------------------------------------------------------------------------------------------------ scores and sums are exact
@pytest.mark.parametrize("dims", X.DIMS2 + X.DIMS3)
@pytest.mark.parametrize("design", X.DESIGNS)
def test_scores_are_exact_multiples_of_G(design, dims):
    Tq, q_pos0 = 5, 700
    Tk = q_pos0 + Tq
    c = X.build_case(design, 2, 2, Tq, q_pos0, Tk, dims)
    s = X.scores_int(c["q"], c["k"])                                    # int64
    assert torch.equal(s, (c["lev"] * X.G)[:, None, None, :].expand_as(s))
    assert bool((s % X.G == 0).all()) and int(s.abs().max()) < (1 << 24) * X.G
    # fp32 in two summation orders, and per-dim partial sums: all equal the int64 value
    qf, kf = c["q"].float(), c["k"].float()
    fwd = torch.einsum("bihd,bjhd->bhij", qf, kf)
    rev = torch.einsum("bihd,bjhd->bhij", qf.flip(-1), kf.flip(-1))
    assert torch.equal(fwd.double(), s.double()) and torch.equal(rev.double(), s.double())
    part = torch.zeros_like(s)
    for d in dims:
        part = part + c["q"][..., d].double().to(torch.int64).permute(0, 2, 1)[..., None] * c["k"][..., d].double().to(torch.int64).permute(0, 2, 1)[:, :, None, :]
        assert bool((part % X.G == 0).all()) and int(part.abs().max()) < (1 << 24) * X.G
    assert torch.equal(part, s)
    # the entries themselves are bf16 integers (a round trip through fp64 integers is the identity)
    for t in (c["q"], c["k"]):
        assert torch.equal(t.double(), t.double().round()) and torch.isfinite(t.float()).all()
    used = (c["q"].abs().amax((0, 1, 2)) > 0) | (c["k"].abs().amax((0, 1, 2)) > 0)
    assert set(used.nonzero().flatten().tolist()) <= set(dims)


def test_three_dim_keys_reach_the_long_cache():
    j = torch.tensor([0, 4095, 4096, 70000, 131071, 262143])
    dig, w = X.key_digits(j, 3), X.q_weights(3)
    assert torch.equal(sum(d * wi for d, wi in zip(dig, w)), j * X.G)
    assert all(int(d.max()) <= 256 for d in dig) and all(float(torch.tensor(float(wi)).to(BF)) == wi for wi in w)
    assert int((j * X.G).max()) < (1 << 24) * X.G
    assert X.G * X.C_LOG2 >= 150 and X.G > X.W_THRP


def test_split_maps():
    assert X.stream_split_counts(130, 4) == [64, 64, 2, 0] and X.stream_split_counts(8229, 4) == [2085, 2048, 2048, 2048]
    assert X.mfma_split_counts(2100, 7) == [320, 320, 320, 320, 320, 320, 180] and X.mfma_split_counts(65, 64) == [64, 1] + [0] * 62
    for n in (1, 64, 65, 2051, 8229):
        for s in (1, 3, 4, 7, 64, 128):
            assert sum(X.stream_split_counts(n, s)) == n == sum(X.mfma_split_counts(n, s))


# ------------------------------------------------------------------------------------------------ the judge on wrong key sets
def _verdict(c, wrong_mult=None, edit=None):
    """Judge the output a kernel with the given defect would return (expected() on the wrong multiplicities, rounded to bf16 as the
    kernels' store does) against the true expectation.  -> (Verdict, affected [B, nq]: rows whose multiset differs)."""
    ref, single = X.expected(c["lev"], c["v"], c["mult"])
    wm = c["mult"] if wrong_mult is None else wrong_mult
    wrong = X.expected(c["lev"], c["v"], wm)[0].to(BF)
    if edit is not None:
        wrong = edit(wrong)
    return X.judge(wrong, ref, single), (wm != c["mult"]).any(-1)


def _seams(c, q_pos0, Tk):
    return [t for t in (0, 63, 64, 127, 128, q_pos0 - 1, q_pos0, q_pos0 + 1, Tk - 1) if 0 <= t < Tk]


PREFILL = (200, 70, 0)


@pytest.mark.parametrize("design", X.DESIGNS)
def test_judge_passes_the_true_key_sets(design):
    c, _ = _case(design, PREFILL)
    ver, _ = _verdict(c)
    assert ver.ok and ver.n_bad == 0 and ver.n_allowed == 0


@pytest.mark.parametrize("shift", [1, -1])
@pytest.mark.parametrize("design", ["U", "D", "S"])
def test_judge_fails_every_row_of_a_wrong_limit(design, shift):
    """A limit of +1 / -1.  U and D: every row whose key set changes (the last row of a +1 stays: Tk clamps it; row 0 at position 0 of
    a -1 would be empty and is not built).  S: every row whose limit crosses a planted key or that still returns the U mean."""
    c, q_pos0 = _case(design, PREFILL)
    Tq, Tk = c["q"].shape[1], c["k"].shape[1]
    wm = X.causal_mult(2, Tq, Tk, q_pos0, shift=shift)
    ver, affected = _verdict(c, wm)
    if design == "S":
        ref, _ = X.expected(c["lev"], c["v"], c["mult"])
        affected = (X.expected(c["lev"], c["v"], wm)[0] != ref).any(-1).any(-1)
    assert int(affected.sum()) >= (Tq - 1 if design != "S" else 8)
    assert torch.equal(ver.bad, affected), (int(ver.bad.sum()), int(affected.sum()))


@pytest.mark.parametrize("times", [0, 2])
def test_judge_fails_every_row_of_a_dropped_or_doubled_key_U(times):
    """One key dropped (x 0) / counted twice (x 2) at each seam, V_hist: EVERY row that sees the key fails.  A row of one key cannot show
    its duplicate (2 v / 2 = v): key 0's doubling is judged on the rows from the second on."""
    c, q_pos0 = _case("U", PREFILL)
    Tk = c["k"].shape[1]
    for t in _seams(c, q_pos0, Tk):
        wm = c["mult"].clone()
        wm[:, :, t] *= times
        ver, affected = _verdict(c, wm)
        if times == 2:
            affected &= c["mult"].sum(-1) >= 2
        assert int(affected.sum()) > 0 and torch.equal(ver.bad, affected), (t, int(ver.bad.sum()), int(affected.sum()))


@pytest.mark.parametrize("design", ["D", "S"])
def test_judge_fails_every_row_that_loses_its_winner(design):
    """D / S with one key dropped at each seam: every row whose winning key it was returns another V row (or the U mean) and fails; the
    rows that only held it at weight 0 are untouched by construction."""
    c, q_pos0 = _case(design, PREFILL)
    Tk = c["k"].shape[1]
    ref, _ = X.expected(c["lev"], c["v"], c["mult"])
    hit = 0
    for t in _seams(c, q_pos0, Tk):
        wm = c["mult"].clone()
        wm[:, :, t] = 0
        if bool((wm.sum(-1) == 0).any()):
            continue                                                     # (key 0 of a row at position 0: the row would be empty)
        ver, _ = _verdict(c, wm)
        affected = (X.expected(c["lev"], c["v"], wm)[0] != ref).any(-1).any(-1)
        hit += int(affected.sum())
        assert torch.equal(ver.bad, affected), t
    assert hit > 0


@pytest.mark.parametrize("design", ["U", "D", "S"])
def test_judge_fails_every_row_of_a_dropped_tile(design):
    c, q_pos0 = _case(design, PREFILL)
    wm = c["mult"].clone()
    wm[:, :, 64:128] = 0
    ver, affected = _verdict(c, wm)
    if design != "U":
        ref, _ = X.expected(c["lev"], c["v"], c["mult"])
        affected = (X.expected(c["lev"], c["v"], wm)[0] != ref).any(-1).any(-1)
    assert int(affected.sum()) > 0 and torch.equal(ver.bad, affected)


@pytest.mark.parametrize("design", X.DESIGNS)
def test_judge_fails_every_row_of_swapped_heads_and_batch_rows(design):
    c, _ = _case(design, PREFILL)
    every = torch.ones_like(c["mult"][:, :, 0], dtype=torch.bool)
    assert torch.equal(_verdict(c, edit=lambda o: o.flip(2))[0].bad, every)
    assert torch.equal(_verdict(c, edit=lambda o: o.flip(0))[0].bad, every)


@pytest.mark.parametrize("design", ["U", "D", "S"])
def test_judge_fails_a_prefix_one_key_short(design):
    """Shared prefix of P keys taken one short (key P - 1 lost).  U (V_hist counts run across the seam): EVERY row fails.  D and S: every
    query sits at or behind P and key P outranks P - 1, so no row's winner changes -- asserted, so that nobody credits them with this."""
    P, Tq, B = 64, 129, 3
    c = X.build_case(design, B, 2, Tq, P, P + Tq, X.DIMS2[2], shared_prefix=P)
    assert torch.equal(c["k"][0, :P], c["k"][2, :P]) and torch.equal(c["v"][0, :P], c["v"][1, :P])
    wm = c["mult"].clone()
    wm[:, :, P - 1] = 0
    ver, affected = _verdict(c, wm)
    if design == "U":
        assert bool(affected.all()) and torch.equal(ver.bad, affected)
    else:
        ref, _ = X.expected(c["lev"], c["v"], c["mult"])
        affected = (X.expected(c["lev"], c["v"], wm)[0] != ref).any(-1).any(-1)
        assert torch.equal(ver.bad, affected) and int(affected.sum()) == 0
    if design == "S":
        assert P - 1 in c["planted"][0] and P in c["planted"][0]


def test_judge_counts_the_allowance_and_caps_it():
    """An element on the wrong side of a boundary it is NOT within 2^-21 of fails; more than 0.1 % on the allowance fails the case."""
    ref = torch.full((1, 1, 1, 128), 1.0 + 2.0 ** -8 + 2.0 ** -22, dtype=torch.float64)      # just above the midpoint of 1 and 1 + 2^-7
    single = torch.zeros(1, 1, dtype=torch.bool)
    hi, lo = torch.full((1, 1, 1, 128), 1.0 + 2.0 ** -7).to(BF), torch.ones(1, 1, 1, 128, dtype=BF)
    assert X.judge(hi, ref, single).ok
    ver = X.judge(lo, ref, single)
    assert ver.n_bad == 0 and ver.n_allowed == 128 and not ver.ok                             # all 128 on the allowance: over the cap
    far = torch.full((1, 1, 1, 128), 1.0 + 2.0 ** -8 + 2.0 ** -12, dtype=torch.float64)
    assert X.judge(lo, far, single).n_bad == 128
    assert X.judge(torch.full((1, 1, 1, 128), float("nan")).to(BF), ref, single).n_bad == 128
    # exact rows: one pattern off fails unless the case allows the adjacent pattern for that row
    one = torch.ones(1, 1, dtype=torch.bool)
    v = torch.full((1, 1, 1, 128), 3.0, dtype=torch.float64)
    off = (v.to(BF).view(torch.int16) + 1).view(BF)
    assert X.judge(off, v, one).n_bad == 128
    ver = X.judge(off, v, one, adjacent_rows=one)
    assert ver.n_bad == 0 and ver.n_adjacent == 128
    assert X.judge((v.to(BF).view(torch.int16) + 2).view(BF), v, one, adjacent_rows=one).n_bad == 128
