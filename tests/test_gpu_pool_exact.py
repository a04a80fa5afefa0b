"""GPU (-m gpu): the masked row pooling (csrc/pool.hip, HipOps.pool_rows) on inputs whose result is exact, in every register plan.

x holds bf16 integers in [-8, 8], a hash of (row, column) so that every row differs (tests/select_ref.py; pinned on the CPU by
tests/test_select_ref_host.py): a column sum over up to 3,000 rows stays below 2^24, so the kernel's fp32 sums are exact in any order
and the output says WHICH rows were pooled -- mode last is the row bit for bit, mode mean is float32(sum) * (1.0f / n): bit for bit
where n is a power of two, within the two roundings 2^-23 abs(ref) elsewhere.  Rows outside every range hold 1e4.  Widths 8 / 264 /
520 / 1032 / 2056 / 4096 reach pool_strip_kernel<1 | 1 | 2 | 4 | 8 | 8> with the `idx < nvec` guard false inside a pass.
With the fused norm the yardstick is fp64 per ELEMENT: ((L + 4) 2^-24 + 2e-6) A_d (select_ref.pool_norm_bound)."""
import pytest
import torch

import select_ref as SR

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_CACHE = {}


def ops():
    from evo_amd.ops import default_ops
    return default_ops()


def ragged(D):
    """The ragged batch of B = 14 at width D, built once: (x [M, D], ranges, fp64 references by mode)."""
    if D not in _CACHE:
        ranges, M, inside = SR.ragged_layout(SR.POOL_LENGTHS)
        x = SR.pool_int_rows(M, D, device=DEV)
        x[~inside.to(DEV)] = SR.OUTSIDE
        _CACHE[D] = (x, ranges, {m: SR.pool_exact_ref(x, ranges, m) for m in ("mean", "last")})
    return _CACHE[D]


def check_exact(got, ref, ranges, mode, what):
    assert got.dtype == torch.float32 and got.shape == ref.shape
    g = got.double()
    for b, (a, n) in enumerate(ranges):
        if mode == "last" or SR.is_pow2(n):
            assert torch.equal(g[b], ref[b]), (what, mode, b, a, n, int((g[b] != ref[b]).sum()))
        else:
            err = (g[b] - ref[b]).abs()
            assert bool((err <= 2.0 ** -23 * ref[b].abs()).all()), (what, b, a, n, float((err / ref[b].abs().clamp(min=1e-30)).max()))


@pytest.mark.parametrize("D", SR.POOL_WIDTHS)
def test_pool_exact_sums_ragged_batch_and_ranges_alone(D):
    x, ranges, ref = ragged(D)
    M = x.shape[0]
    assert ranges[0][0] == 0 and ranges[-1][0] + ranges[-1][1] == M        # a range from row 0, a range to row M - 1
    wide = torch.full((M, D + 72), SR.OUTSIDE, dtype=torch.bfloat16, device=DEV)
    wide[:, :D] = x
    for mode in ("mean", "last"):
        got = ops().pool_rows(x, ranges, mode=mode)                         # B = 14: 74 strips, most of them empty for the short ranges
        check_exact(got, ref[mode], ranges, mode, "ragged")
        for b, rg in enumerate(ranges):                                    # B = 1: n = 3,000 gives 188 strips, 11 or 12 slabs per finish wave
            alone = ops().pool_rows(x, [rg], mode=mode)
            check_exact(alone, ref[mode][b:b + 1], [rg], mode, "alone")
            assert torch.equal(alone[0], got[b])
        assert torch.equal(ops().pool_rows(wide[:, :D], ranges, mode=mode), got)     # a pitch above D
    # B = 300 overlapping ranges of 40 rows: 3 strips of 14 / 14 / 12 rows from POOL_WORKGROUPS / B
    assert SR.pool_strips(300, 40) == 3
    over = [(7 * b, 40) for b in range(299)] + [(M - 40, 40)]
    for mode in ("mean", "last"):
        check_exact(ops().pool_rows(x, over, mode=mode), SR.pool_exact_ref(x, over, mode), over, mode, "overlapping")


@pytest.mark.parametrize("D", [8, 1032, 4096])
def test_pool_tensor_ranges_nan_exactly_in_the_invalid_rows(D):
    x, ranges, ref = ragged(D)
    M = x.shape[0]
    bad = {1: (-1, 5), 4: (17, 0), 6: (M - 4, 5), 9: (M, 1), 15: (3, -2)}   # first = -1, n = 0, first + n = M + 1, first = M, n < 0
    pairs, good = [], []
    it = iter(ranges)
    for i in range(len(ranges) + len(bad)):
        if i in bad:
            pairs.append(bad[i])
        else:
            pairs.append(next(it))
            good.append(i)
    rg = torch.tensor(pairs, dtype=torch.int64, device=DEV)
    for mode in ("mean", "last"):
        got = ops().pool_rows(x, rg, mode=mode)
        torch.cuda.synchronize()
        assert bool(torch.isnan(got[sorted(bad)]).all()) and not bool(torch.isnan(got[good]).any())
        clean = ops().pool_rows(x, torch.tensor(ranges, dtype=torch.int64, device=DEV), mode=mode)
        assert torch.equal(got[good], clean)
        check_exact(clean, ref[mode], ranges, mode, "tensor ranges")
        assert torch.equal(clean, ops().pool_rows(x, ranges, mode=mode))


@pytest.mark.parametrize("D", SR.NORM_WIDTHS)
def test_pool_norm_per_element_bound(D):
    ranges, M, inside = SR.ragged_layout(SR.NORM_LENGTHS)
    x, scale = SR.pool_norm_rows(M, D, device=DEV)
    x[~inside.to(DEV)] = SR.OUTSIDE
    ref, A = SR.pool_norm_ref(x, ranges, scale, 1e-6)
    worst = 0.0
    for what, groups in (("ragged", [ranges]), ("alone", [[rg] for rg in ranges])):
        for rgs in groups:
            got = ops().pool_rows(x, rgs, scale=scale, eps=1e-6, mode="mean").double()
            n_strips = SR.pool_strips(len(rgs), max(n for _, n in rgs))
            for i, (a, n) in enumerate(rgs):
                b = ranges.index((a, n))
                bound = SR.pool_norm_bound(A[b], n, n_strips)
                err = (got[i] - ref[b]).abs()
                ratio = float((err / bound.clamp(min=1e-300)).max())
                worst = max(worst, ratio)
                assert bool((err <= bound).all()), (what, D, a, n, n_strips, ratio, int((err / bound.clamp(min=1e-300)).argmax()))
    last = ops().pool_rows(x, ranges, scale=scale, eps=1e-6, mode="last").double()
    lr = [(a + n - 1, 1) for a, n in ranges]
    lref, lA = SR.pool_norm_ref(x, lr, scale, 1e-6)
    lerr = (last - lref).abs()
    lbound = (4 * 2.0 ** -24 + SR.RSTD_ERR) * lA
    worst_last = float((lerr / lbound.clamp(min=1e-300)).max())
    print(f"[pool exact norm D={D}] worst err / bound: mean {worst:.3f}, last {worst_last:.3f}")
    assert bool((lerr <= lbound).all()), worst_last
