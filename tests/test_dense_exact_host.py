"""CPU: pins tests/dense_exact.py -- the data of tests/test_gpu_dense_exact.py really are exact, and they can see what the bounds they
replace cannot.  The constructors hash (row, column, seed), so a tensor made here is the top-left block of the tensor the GPU module
makes with the same seed: these checks run on blocks of the very operands the kernels get."""
import pytest
import torch

import dense_exact as DX

KS = DX.all_reductions()


def test_every_shape_of_the_gpu_module_keeps_its_sums_below_2_to_24():
    """sum |x w| <= 4 * 2 * K; the row factor (<= 8) and the bias / residual (units of 1/4, |.| < 72) stay far inside fp32 too:
    (8 * 8 K + 72) * 4 quarter units < 2^24 for the shapes with a row factor, (8 K + 72) * 4 < 2^24 for all."""
    assert KS[-1] == DX.K_MAX == 11008 and KS[0] == 64
    for K in KS:
        assert 8 * K < 2 ** 24 and (8 * K + 72) * 4 < 2 ** 24
    for M, N, K in DX.ROW_SCALE:
        assert (8 * 8 * K + 72) * 8 < 2 ** 24                           # (2^-3 S is a multiple of 1/8)
    for B, T, N, K in DX.LINEAR_T:
        assert (8 * 8 * K + 72) * 8 < 2 ** 24
    for M, I, K in DX.GATED:
        assert (8 * 8 * K) * 2 ** 7 * 8 < 2 ** 24 * 2 ** 7              # W1 in units of 2^-7: 8 K units < 2^24, times the row factor's 2^-3 .. 2^3
    for M, N, K in DX.SUMSQ:
        assert 128 * 24 ** 2 == 73728 < 2 ** 24                          # a 128-column strip of squares of integers |y| <= 24


@pytest.mark.parametrize("K", KS)
def test_fp32_equals_fp64_in_two_summation_orders_and_operands_are_bf16(K):
    M, N = 64, 256
    x, w, b, r = DX.make_x(M, K), DX.make_w(N, K), DX.make_bias(N), DX.make_residual(M, N)
    for t, lo, hi, unit in ((x, -4, 4, 1), (w, -2, 2, 1), (b, -8, 8, 4), (r, -63.75, 63.75, 4)):
        d = t.double()
        assert t.dtype == torch.bfloat16 and torch.equal(d.float().bfloat16().double(), d)            # survives the bf16 round trip
        assert float(d.min()) >= lo and float(d.max()) <= hi and torch.equal(d * unit, (d * unit).round())
    assert float(x.double().min()) == -4 and float(x.double().max()) == 4 and float(w.double().min()) == -2 and float(w.double().max()) == 2
    # every row and every column different
    assert len({tuple(v.tolist()) for v in x.double()}) == M and len({tuple(v.tolist()) for v in w.double()}) == N
    assert len({tuple(v.tolist()) for v in x.double().t()[:64]}) == 64 and len({tuple(v.tolist()) for v in r.double().t()}) == N
    s = DX.exact_sum(x, w, b, r)
    f = x.float() @ w.float().t() + b.float() + r.float()
    fr = x.float().flip(-1) @ w.float().flip(-1).t() + (b.float() + r.float())
    assert torch.equal(f.double(), s) and torch.equal(fr.double(), s)
    assert torch.equal(DX.expected(x, w, b, r).double(), s.float().bfloat16().double())
    # the gate's weights: W1 in units of 2^-7
    w12 = DX.make_gate_weights(N // 2, K)
    assert torch.equal(w12.double().float().bfloat16().double(), w12.double())
    assert torch.equal(w12[:N // 2].double() * 128, (w12[:N // 2].double() * 128).round()) and float(w12[:N // 2].double().abs().max()) == 2.0 ** -6
    s12 = DX.exact_product(x, w12)
    assert torch.equal((x.float() @ w12.float().t()).double(), s12) and torch.equal((x.float().flip(-1) @ w12.float().flip(-1).t()).double(), s12)


@pytest.mark.parametrize("K", KS)
def test_the_sums_exercise_the_rounding(K):
    """More than 10 % of the exact sums are no bf16 number and more than 5 % are exact round-to-nearest-even TIES, at every K used; a
    second rounding shows: the residual added after a rounding of x w^T + b gives another pattern on more than 1 % of the elements at
    every K, the bias added after a rounding of x w^T on more than 1 % from K = 2,048 on (below, |x w^T| < 256 is itself a bf16 number);
    truncation instead of rounding shows on more than 5 %."""
    M, N = 128, 512
    x, w, b, r = DX.make_x(M, K), DX.make_w(N, K), DX.make_bias(N), DX.make_residual(M, N)
    S = DX.exact_product(x, w)
    s = DX.exact_sum(x, w, b, r, S=S)
    inexact, ties, trunc = DX.shares(s)
    print(f"[dense_exact host] K {K}: not representable {inexact:.3f}, ties {ties:.3f}, truncation differs {trunc:.3f}")
    assert inexact > 0.10 and ties > 0.05 and trunc > 0.05
    want = DX.expected(x, w, b, r, S=S)
    late_r = (DX.expected(x, w, b, S=S).float() + r.float()).bfloat16()
    assert DX.mismatches(late_r, want)[0] > 0.01 * want.numel()
    assert DX.mismatches(DX.truncate_bf16(s), want)[0] > 0.05 * want.numel()
    if K >= 2048:
        late_b = (S.float().bfloat16().float() + b.float()).bfloat16()
        n = DX.mismatches(late_b, DX.expected(x, w, b, S=S))[0]
        print(f"[dense_exact host] K {K}: bias after the rounding differs on {n / want.numel():.3f}")
        assert n > 0.01 * want.numel()


@pytest.mark.parametrize("K", sorted({k for _, k in DX.DOT2 + DX.DOT2_LE4 + DX.SKINNY_MFMA + DX.SKINNY_NW + DX.GATE_SMALL} | {s[2] for s in DX.SPLITK}))
def test_sixteenth_unit_x_is_exact_too(K):
    """The weight-streaming forms' second data set (x in multiples of 1/16): exact in bf16, (8 K + 72) * 16 units < 2^24, fp32 == fp64 in two
    summation orders, plain and against the gate's weights (units of 2^-11)."""
    assert (8 * K + 72) * 16 < 2 ** 24
    M, N = 64, 256
    x, w, b, r = DX.make_x(M, K, unit=16), DX.make_w(N, K), DX.make_bias(N), DX.make_residual(M, N)
    d = x.double()
    assert torch.equal(d.float().bfloat16().double(), d) and torch.equal(d * 16, (d * 16).round()) and float(d.min()) == -4 and float(d.max()) == 4
    assert float(((d * 16) % 2 != 0).double().mean()) > 0.4                              # odd sixteenths are common
    assert len({tuple(v.tolist()) for v in d}) == M
    s = DX.exact_sum(x, w, b, r)
    assert torch.equal((x.float() @ w.float().t() + b.float() + r.float()).double(), s)
    assert torch.equal((x.float().flip(-1) @ w.float().flip(-1).t() + (b.float() + r.float())).double(), s)
    w12 = DX.make_gate_weights(N // 2, K)
    s12 = DX.exact_product(x, w12)
    assert torch.equal((x.float() @ w12.float().t()).double(), s12) and torch.equal((x.float().flip(-1) @ w12.float().flip(-1).t()).double(), s12)
    inexact, ties, trunc = DX.shares(s)
    assert inexact > 0.10 and ties > 0.05


@pytest.mark.parametrize("K", [288, 4096])
def test_partial_sums_through_bf16_show_on_the_sixteenth_unit_data(K):
    """Why the second data set exists: eight partial sums that cross LDS in bf16 (dense_exact.through_bf16_partials) leave the INTEGER data
    almost untouched -- a partial sum of integers below 256 is a bf16 number -- and change more than 5 % of the elements of the
    sixteenth-unit data at both reduction lengths."""
    M, N = 64, 512
    w, b, r = DX.make_w(N, K), DX.make_bias(N), DX.make_residual(M, N)
    share = {}
    for unit in DX.X_UNITS:
        x = DX.make_x(M, K, unit=unit)
        share[unit] = DX.mismatches(DX.through_bf16_partials(x, w, b, r), DX.expected(x, w, b, r))[0] / (M * N)
    print(f"[dense_exact host] K {K}: bf16 partial sums change {share[1]:.4f} of the elements on integer x, {share[16]:.4f} on sixteenth-unit x")
    assert share[16] > 0.05
    if K == 288:
        assert share[1] == 0.0


def test_hash_does_not_depend_on_the_shape():
    assert torch.equal(DX.make_w(300, 4096)[:64, :192], DX.make_w(64, 192))
    assert torch.equal(DX.make_residual(70, 513)[:9, :37], DX.make_residual(9, 37))
    assert not torch.equal(DX.make_x(8, 64, seed=1), DX.make_x(8, 64, seed=2))


@pytest.mark.parametrize("K", [256, 1024, 4096])
def test_norm_rows_are_exact_in_emulated_fp32(K):
    """RMSNorm of make_norm_rows in numpy float32, statement by statement: sum of squares K 4^a, the factor 2^-a, the row g x 2^-a."""
    M = 9
    x, a = DX.make_norm_rows(M, K)
    g = DX.make_norm_scale(K)
    assert set(a.tolist()) == set(DX.NORM_EXPS)
    xd = x.double() * torch.ldexp(torch.ones(M, dtype=torch.float64), (-a).to(torch.int32))[:, None]
    assert bool(((xd.abs() == 1).sum(-1) == K // 2).all()) and bool(((xd.abs() == 2).sum(-1) == K // 8).all()) and bool(((xd == 0).sum(-1) == 3 * K // 8).all())
    assert torch.equal(x.double().pow(2).sum(-1), K * 4.0 ** a.double())
    assert set(g.double().tolist()) == {1.0, 2.0, 3.0}
    out, inv = DX.rmsnorm_fp32_emulated(x, g)
    assert torch.equal(inv.double(), 2.0 ** -a.double())
    want = DX.norm_rows_expected(x, g, a)
    assert torch.equal(out.double(), want.double()) and float(want.double().abs().max()) == 6 and torch.equal(want.double(), want.double().round())
    assert len({tuple(v.tolist()) for v in x.double()}) == M
    # the dense layer behind it stays exact: |n| <= 6, |w| <= 2
    w = DX.make_w(64, K)
    assert torch.equal((want.float() @ w.float().t()).double(), DX.exact_product(want, w))


def test_sum_of_squares_inputs():
    M, N, K = 70, 256, 192
    x, w, r = DX.make_sparse_x(M, K), DX.make_w(N, K), DX.make_int_residual(M, N)
    assert bool(((x != 0).sum(-1) == 8).all()) and float(x.double().abs().max()) == 1
    y = DX.expected(x, w, None, r).double()
    assert torch.equal(y, DX.exact_sum(x, w, None, r)) and float(y.abs().max()) <= 24      # the stored rows are the exact integers
    ss = y.pow(2).view(M, N // 128, 128).sum(-1)
    assert float(ss.max()) <= 73728 and torch.equal(ss.float().double(), ss)
    assert len({tuple(v.tolist()) for v in x.double()}) == M


def test_row_factors_are_powers_of_two_and_differ():
    p = DX.make_pow2_rows(512)
    assert set(p.tolist()) == {2.0 ** e for e in range(-3, 4)} and bool((p[1:] != p[:-1]).float().mean() > 0.7)
