"""CPU: pins tests/select_ref.py -- the constructors' invariants and the predictions that tests/test_gpu_sample_regimes.py and
tests/test_gpu_pool_exact.py judge the kernels by -- where no GPU is needed: the flat-row prediction order[floor(u n)] equals the written
specification (evo_amd/sh/sample.py: sample_seeded) on every row the GPU test launches, the top-p cut keeps its distance from every
integer, both exclusion shares stay under their caps, and the pooling references equal plain fp64 torch."""
import numpy as np
import pytest
import torch

import select_ref as SR
from evo_amd.sh import sample as H


def test_flat_rows_hold_what_they_promise():
    c = SR.flat_case()
    rows, kind = c["rows"], c["kind"]
    assert rows.shape == (8192, 512) and torch.equal(rows.bfloat16().float(), rows)
    fin = torch.isfinite(rows)
    assert float(rows[fin].abs().max()) <= 64 and bool(fin[:, SR.A_ID].all())
    # expf((v - v0) / 2^40) is exactly 1.0f over the whole range of the rows (fp32 numpy)
    d = np.float32(-128.0) / np.float32(SR.FLAT_T)
    assert np.exp(d, dtype=np.float32) == np.float32(1.0) and np.exp(np.float32(-40.0) / np.float32(SR.FLAT_T), dtype=np.float32) == 1.0
    for name in ("asc", "desc", "bitrev", "shuf"):
        r = rows[kind == SR.KINDS.index(name)]
        assert r.shape[0] == 512
        srt = torch.sort(r, dim=1)[0]
        assert bool((torch.diff(srt, dim=1) > 0).sum(1).eq(510).all())                # 511 distinct values: -0 and +0 are one
        assert bool((r == 0).sum(1).eq(2).all()) and bool((torch.signbit(r) & (r == 0)).sum(1).eq(1).all())
        assert bool((r == SR.SUBNORMAL).sum(1).eq(1).all()) and bool((r < 0).any(1).all())
        if name == "asc":
            assert bool((torch.diff(r, dim=1) >= 0).all())
        elif name == "desc":
            assert bool((torch.diff(r, dim=1) <= 0).all())
        elif name == "bitrev":
            assert bool((torch.diff(r[:, SR.bit_reverse9(torch.arange(512))], dim=1) >= 0).all())
    assert sorted(SR.bit_reverse9(torch.arange(512)).tolist()) == list(range(512)) and int(SR.bit_reverse9(torch.tensor([1]))[0]) == 256
    const = rows[kind == SR.KINDS.index("const")]
    assert bool((const == const[:, :1]).all()) and const[:, 0].unique().numel() == 13
    holes = (~fin).sum(1)
    assert set(holes[kind >= 12].tolist()) == {1, 100, 511} and int(holes[kind < 12].max()) == 0
    for k in (12, 13, 14, 15):
        assert set(holes[kind == k].tolist()) == {1, 100, 511}
    ints = rows[kind < 5]
    assert torch.equal(ints, ints.round()) and float(ints.min()) == -6 and float(ints.max()) == 6
    # every kind meets every top_k and every top_p; every top_k meets every top_p
    seen_k = {(int(a), int(b)) for a, b in zip(kind.tolist(), c["top_k"].tolist())}
    assert seen_k == {(a, b) for a in range(16) for b in SR.ALL_KS}
    seen_p = {(int(a), float(b)) for a, b in zip(c["top_k"].tolist(), c["top_p"].tolist())}
    assert len(seen_p) == len(SR.ALL_KS) * 3
    assert len({(int(a), float(b)) for a, b in zip(kind.tolist(), c["top_p"].tolist())}) == 16 * 3
    assert bool((c["temperature"][c["top_k"] != 1] == SR.FLAT_T).all())


def test_top_p_cut_keeps_its_distance_from_every_integer():
    assert np.float32(1.0) - np.float32(SR.P_CUT) == np.float32(0.6180340052)
    d64, n64 = SR.cut_distance()
    d32, n32 = SR.cut_distance(float(np.float32(1.0) - np.float32(SR.P_CUT)))           # the kernel's 1.0f - p
    print(f"[select ref] min distance of n (1 - p) from an integer: {d64:.4e} at n = {n64} (fp32 1 - p: {d32:.4e} at n = {n32})")
    assert d64 >= SR.CUT_MARGIN and d32 >= SR.CUT_MARGIN and n64 == n32 == 377
    assert SR.CUT_MARGIN >= 40 * 512 * 2.0 ** -24 * 0.9                                  # ~40 x the rounding of thr = (1 - p) Z at Z = 512
    # ... so the number of tokens cut is the same in fp32 and fp64 for every n
    n = torch.arange(1, 513)
    q32 = float(np.float32(1.0) - np.float32(SR.P_CUT))
    assert torch.equal(torch.floor(n.double() * (1.0 - SR.P_CUT)), torch.floor(n.double() * q32))


@pytest.mark.parametrize("mask_name", SR.MASKS)
def test_flat_prediction_equals_the_specification_on_every_row(mask_name):
    c = SR.flat_case()
    mask = SR.flat_mask(mask_name)
    tok, out, n, _ = SR.flat_expected(mask_name)
    share = out.float().mean().item()
    drew = c["top_k"] != 1
    print(f"[select ref] mask {mask_name}: rows left out {100 * share:.3f} %, n kept {int(n[drew].min())} .. {int(n[drew].max())}")
    assert share <= SR.U_CAP
    if mask is not None:
        assert bool(mask[tok].all())
    if mask_name == "one":
        assert bool((tok == SR.A_ID).all())
    checked = 0
    for k in SR.ALL_KS:
        for p in SR.TOP_PS:
            idx = torch.nonzero((c["top_k"] == k) & (c["top_p"] == np.float32(p))).flatten()
            assert idx.numel() > 0
            T = 0.7 if k == 1 else SR.FLAT_T
            spec = H.sample_seeded(c["rows"][idx], k, p, T, SR.FLAT_SEED, c["stream"][idx].numpy(), c["count"][idx].numpy(), allowed=mask)
            _, _, n_spec = H.seeded_distribution(c["rows"][idx], k, p, T, mask)
            assert torch.equal(n_spec, n[idx]), (k, p)                                   # the kept set's size: every row, no exclusion
            keep = ~out[idx]
            assert torch.equal(spec[keep], tok[idx][keep]), (k, p)
            checked += int(keep.sum())
    assert checked == int((~out).sum())
    if mask_name == "none":
        tied = n[(c["top_k"] == 65) & (c["top_p"] != np.float32(SR.P_CUT)) & (c["kind"] < 5)]
        assert int(tied.min()) >= 65 and float((tied > 65).float().mean()) > 0.9         # the tie regime: more than k tokens stay


def test_keying_values_have_high_words_and_predict_through_the_specification():
    j = np.arange(2048, dtype=np.int64)
    for name, f in list(SR.STREAMS64.items())[1:] + list(SR.COUNTS64.items())[1:]:
        v = np.asarray(f(j), dtype=np.int64)
        assert bool(((v.astype(np.uint64) >> np.uint64(32)) != 0).all()), name
        assert bool((SR.low32(v) >= 0).all()) and bool((SR.low32(v) < 2 ** 32).all())
    assert [SR.low32(s) for s in SR.SEEDS64] == [5, 5, 12345, 0xFFFFFFFF]
    # the u the prediction uses is the specification's, scalar and array forms alike, at the extreme words
    for seed in SR.SEEDS64:
        for st, ct in ((2 ** 62 + 7, 2 ** 40), (-8, 2 ** 32 + 7), (2 ** 32 + 7, 7)):
            a = H.seeded_uniform(seed, st, ct)
            b = H.seeded_uniform(seed, np.array([st], dtype=np.int64), np.array([ct], dtype=np.int64))[0]
            assert a == b and 0.0 < a < 1.0
            assert a != H.seeded_uniform(SR.low32(seed), st, ct) or seed == 5
            for lo_st, lo_ct in ((int(SR.low32(np.int64(st))), ct), (st, int(SR.low32(np.int64(ct))))):
                assert (lo_st, lo_ct) == (st, ct) or a != H.seeded_uniform(seed, lo_st, lo_ct)          # a dropped high word shows


@pytest.mark.parametrize("name,f32,settings,logprob", SR.EXTREME_CASES, ids=[c[0] for c in SR.EXTREME_CASES])
def test_extreme_rows_stay_inside_the_undecidable_cap(name, f32, settings, logprob):
    from test_gpu_sample import accept, undecidable
    rows = SR.extreme_rows(name)
    assert rows.shape == (4096, 512) and rows.dtype == (torch.float32 if f32 else torch.bfloat16)
    x = rows.double()
    top = x.topk(3, dim=-1)[0]
    if name == "wide":
        assert float(x.abs().max()) > 2.9e4 and bool((top[:, 0] - top[:, 2] == 1.5).all())
        e = torch.exp((x - top[:, :1]).float())
        assert float(((e == 0) | (e < 2.0 ** -126)).float().mean()) > 0.95             # most terms underflow to 0 or a subnormal
    elif name == "spike":
        assert bool((top[:, 0] == 60).all()) and float(top[:, 1].max()) < 20
    elif name == "top2":
        assert bool((top[:, 0] == top[:, 1]).all())
    stream, count = SR.extreme_keys(4096)
    for k, p, T in settings:
        assert p == 1.0 or T <= 1.2
        share = undecidable(rows, k, p, T, None).float().mean().item()
        print(f"[select ref] {name} k={k} p={p} T={T}: undecidable {100 * share:.2f} %")
        assert share <= SR.UNDECIDABLE_CAP, (name, k, p, T, share)
    # the acceptance rule accepts the specification's own token
    k, p, T = settings[0]
    spec = H.sample_seeded(rows[:512], k, p, T, SR.EXTREME_SEED, stream[:512], count[:512])
    out, bad = accept(rows[:512], spec, k, p, T, None, SR.EXTREME_SEED, stream[:512], count[:512])
    assert int(bad.sum()) == 0


def test_pool_integer_rows_and_layout():
    for D in SR.POOL_WIDTHS:
        M = 6400 if D <= 264 else 700
        x = SR.pool_int_rows(M, D)
        xd = x.double()
        assert x.dtype == torch.bfloat16 and torch.equal(xd, xd.round()) and float(xd.min()) == -8 and float(xd.max()) == 8
        assert torch.unique(xd, dim=0).shape[0] == M                                     # every row differs
        assert torch.equal(x[:50], SR.pool_int_rows(50, D))                              # a function of (row, column) alone
    assert 3000 * 8 < 2 ** 24
    assert [SR.pool_plan_nv(D) for D in SR.POOL_WIDTHS] == [1, 1, 2, 4, 8, 8]
    assert [D // 8 for D in SR.POOL_WIDTHS] == [1, 33, 65, 129, 257, 512]
    assert all((D // 8) % 64 != 0 for D in SR.POOL_WIDTHS[:-1])                          # the idx < nvec guard is false inside a pass
    ranges, M, inside = SR.ragged_layout(SR.POOL_LENGTHS)
    assert len(ranges) == 14 and ranges[0][0] == 0 and ranges[-1][0] + ranges[-1][1] == M
    assert int(inside.sum()) == sum(SR.POOL_LENGTHS) and int((~inside).sum()) == 13 * 3
    # the strip plans the GPU test relies on
    assert SR.pool_strips(14, 3000) == 74 and SR.pool_chunk(1, 74) == 1                   # short ranges: 73 empty strips
    assert SR.pool_strips(1, 3000) == 188 and SR.pool_chunk(3000, 188) == 16              # 188 slabs: 11 or 12 per finish wave
    assert {len(range(w, 188, 16)) for w in range(16)} == {11, 12}
    assert SR.pool_strips(300, 40) == 3 and SR.pool_chunk(40, 3) == 14
    assert SR.pool_adds(3000, 188) == 4 + 2 + 12 + 15
    # the exact reference is plain fp64 torch
    x = SR.pool_int_rows(200, 264)
    rg = [(0, 1), (3, 64), (70, 130)]
    assert torch.equal(SR.pool_exact_ref(x, rg, "mean"), torch.stack([x[a:a + n].double().mean(0) for a, n in rg]))
    assert torch.equal(SR.pool_exact_ref(x, rg, "last"), torch.stack([x[a + n - 1].double() for a, n in rg]))


def test_pool_norm_reference_equals_fp64_torch():
    D = 264
    x, scale = SR.pool_norm_rows(130, D)
    xd = x.double()
    r = torch.arange(130)
    assert bool((xd[r % 25 == 4] == 0).all()) and float(xd[1].abs().max()) > 1e11 and 0 < float(xd[2].abs().max()) < 1e-10
    assert float(xd[3, D // 3].abs()) > 50 * float(xd[3].abs().median())
    rg = [(0, 1), (4, 1), (5, 17), (20, 110)]
    ref, A = SR.pool_norm_ref(x, rg, scale, 1e-6)
    for b, (a, n) in enumerate(rg):
        rows = xd[a:a + n]
        f = rows / (rows.pow(2).mean(1, keepdim=True).sqrt() + 1e-6)
        want = (f * scale.double()).mean(0)
        assert float((ref[b] - want).abs().max()) <= 1e-12 * float(1 + want.abs().max())
        assert bool((A[b] >= ref[b].abs() * (1 - 1e-12)).all())
    assert bool((ref[1] == 0).all()) and bool((A[1] == 0).all())                         # the zero row: 0 * 1e6
    b = SR.pool_norm_bound(A, 110, 7)
    assert torch.equal(b, ((SR.pool_adds(110, 7) + 4) * 2.0 ** -24 + 2e-6) * A)
