"""GPU (-m gpu): the row-invariant dense launches (evo_linear_rowinv_bf16, evo_mlp_gate_rowinv_bf16) at EVERY row
count and EVERY row, at the shapes the 7B step runs.  tests/test_gpu_rowinv.py samples rows 0, M / 2, M - 1 at 13 row counts on the
smallest shape of five routes; a row's accumulator is acc[row / 16] and its x row sits at LDS row 16 t + r16, so a defect confined to one
m tile or to a few lanes of one passes there.  Here:

    shapes       the five layers of the 7B step -- (12288, 4096) [3 waves wide], (4096, 4096) [4 waves, 4 slices of 4 units], (4096, 11008)
                 [4 slices of 10 / 11 / 11 / 11], (512, 4096) [2 waves, 8 slices], the gate I = 11008, K = 4096 in both layouts -- and the
                 smallest shape of every other route: (12288, 256), (512, 2304) [9 units over 8 slices], (4096, 2816) [11 units over 4],
                 (8192, 256), (16384, 256) [2 / 4 waves wide]                                         (tests/rowinv_ref.py: the routing restated)
    rows / M     x = 64 distinct N(0, 1) rows (weights scaled by K^-1/2 at K >= 4096); `alone` = the 64 one-row calls; for every M in
                 1 .. 64 f(x[:M]) == alone[:M] on the whole tensor -- every row at every M; modes plain / bias / residual / both
    index        one fixed permutation of the 64 rows: f(x[perm][:M]) == alone[perm][:M] at M in {1, 16, 17, 32, 33, 48, 49, 64}
    neighbours   the other rows 1e30, then NaN, at M in {17, 33, 49, 64}; the odd rows filled, then the even ones: every row is checked
                 beside poisoned neighbours
    values       the exact designs of tests/dense_exact.py (integers and sixteenths) at the five 7B shapes, M = 64, four modes: 0 bf16
                 patterns differ from the once-rounded exact sum; (4096, 11008) bias + residual at every M.  With the every-M equality
                 on N(0, 1) data this pins the value of every row at every M
    route        the C entry with a caller-owned workspace of 8 M N NaN floats: the number of [M, N] slabs overwritten is the restated
                 slice count, the same at M = 1 and 64, 0 for N >= 8192
    teeth        the DEFAULT ops.linear on the same data, at each 7B shape: some row differs between its one-row call and some M-row call

Every comparison is equality of bf16 bit patterns; nothing here has a tolerance (the gate's value check is rowlocal_ref.gelu_gate_check's
bound, as in tests/test_gpu_rowinv.py)."""
import time

import pytest
import torch

import dense_exact as DX
import rowinv_ref as RI
import rowlocal_ref as RL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODES = [("plain", False, False), ("bias", True, False), ("residual", False, True), ("bias+residual", True, True)]
SHAPES = RI.LINEAR_7B + RI.LINEAR_SMALL
GATES = [RI.GATE_7B]
PERM_MS = [1, 16, 17, 32, 33, 48, 49, 64]
FILL_MS = [17, 33, 49, 64]
PERM = torch.randperm(64, generator=torch.Generator().manual_seed(64)).tolist()
TOTAL = {"launches": 0, "elements": 0, "mismatches": 0, "t0": None}
_DATA, _ALONE = {}, {}


def _ops():
    from evo_amd.ops import default_ops
    ops = default_ops()
    assert ops.supports("row_invariant")
    if TOTAL["t0"] is None:
        TOTAL["t0"] = time.time()
    return ops


def _bits(t):
    return t.contiguous().view(torch.int16)


def _randn(*shape, seed, scale=1.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV, dtype=torch.float32) * scale).to(torch.bfloat16)


def _data(N, K):
    """x [64, K], w [N, K] (x K^-1/2 at K >= 4096), bias [N], residual [64, N]: N(0, 1), made once per shape and never modified."""
    if (N, K) not in _DATA:
        assert PERM != sorted(PERM)
        _DATA[(N, K)] = (_randn(64, K, seed=21), _randn(N, K, seed=22, scale=K ** -0.5 if K >= 4096 else 1.0), _randn(N, seed=23),
                         _randn(64, N, seed=24))
    return _DATA[(N, K)]


def _run(ops, x, w, b, r):
    TOTAL["launches"] += 1
    return ops.linear_residual_rowinv_(r.clone(), x, w, bias=b) if r is not None else ops.linear_rowinv(x, w, b)


def _alone(ops, N, K, mode):
    """The 64 one-row calls of a mode, concatenated -- computed once per (shape, mode), shared by the tests and never modified."""
    if (N, K, mode) not in _ALONE:
        x, w, b, r = _data(N, K)
        _, bias, res = MODES[mode]
        out = torch.cat([_run(ops, x[i:i + 1], w, b if bias else None, r[i:i + 1] if res else None) for i in range(64)])
        assert bool(torch.isfinite(out.float()).all())
        _ALONE[(N, K, mode)] = out
    return _ALONE[(N, K, mode)]


def _same(got, want, what):
    ne = _bits(got) != _bits(want)
    n = int(ne.sum())
    TOTAL["elements"] += got.numel()
    TOTAL["mismatches"] += n
    assert n == 0, f"{what}: {n} of {got.numel()} bf16 patterns differ from the one-row calls, rows {ne.any(1).nonzero().flatten().tolist()[:16]}"


def _gate_data(I, K):
    if ("gate", I, K) not in _DATA:
        w12 = _randn(2 * I, K, seed=26, scale=K ** -0.5)
        _DATA[("gate", I, K)] = (_randn(64, K, seed=25), w12)
    return _DATA[("gate", I, K)]


def _gate_layouts(ops, w12):
    return (("plain", (w12, None)), ("grouped", (None, ops.pack_gate_weights(w12))))


def _gate(ops, x, args):
    TOTAL["launches"] += 1
    return ops.mlp_gate_rowinv(x, *args)


# ================================================================================================ rows do not see M
@pytest.mark.parametrize("N,K", SHAPES)
def test_every_row_at_every_m(N, K):
    ops = _ops()
    x, w, b, r = _data(N, K)
    for mode, (name, bias, res) in enumerate(MODES):
        alone = _alone(ops, N, K, mode)
        for M in RI.EVERY_M:
            _same(_run(ops, x[:M], w, b if bias else None, r[:M] if res else None), alone[:M], f"{N}x{K} {name} M={M}")


@pytest.mark.parametrize("N,K", SHAPES)
def test_rows_do_not_see_their_index(N, K):
    ops = _ops()
    x, w, b, r = _data(N, K)
    xp, rp = x[PERM].contiguous(), r[PERM].contiguous()
    for mode, (name, bias, res) in enumerate(MODES):
        alone = _alone(ops, N, K, mode)[PERM]
        for M in PERM_MS:
            _same(_run(ops, xp[:M].contiguous(), w, b if bias else None, rp[:M].contiguous() if res else None), alone[:M],
                  f"{N}x{K} {name} permuted rows, M={M}")


@pytest.mark.parametrize("N,K", SHAPES)
def test_rows_do_not_see_their_neighbours(N, K):
    """The odd rows filled (1e30, then NaN; x and residual alike), then the even ones: EVERY row that is not filled equals its one-row call."""
    ops = _ops()
    x, w, b, r = _data(N, K)
    idx = torch.arange(64, device=DEV)
    for mode, (name, bias, res) in enumerate(MODES):
        alone = _alone(ops, N, K, mode)
        for M in FILL_MS:
            for parity in (1, 0):
                keep = idx[:M] % 2 != parity
                assert 0 < int(keep.sum()) < M
                for fname, v in (("large", 1e30), ("nan", float("nan"))):
                    xf, rf = torch.full((M, K), v, dtype=torch.bfloat16, device=DEV), torch.full((M, N), v, dtype=torch.bfloat16, device=DEV)
                    xf[keep], rf[keep] = x[:M][keep], r[:M][keep]
                    got = _run(ops, xf, w, b if bias else None, rf if res else None)
                    _same(got[keep], alone[:M][keep], f"{N}x{K} {name} M={M}, rows of parity {parity} filled with {fname}")


@pytest.mark.parametrize("I,K", GATES)
def test_gate_every_row_at_every_m(I, K):
    ops = _ops()
    x, w12 = _gate_data(I, K)
    idx = torch.arange(64, device=DEV)
    xp = x[PERM].contiguous()
    outs = []
    for lname, args in _gate_layouts(ops, w12):
        alone = torch.cat([_gate(ops, x[i:i + 1], args) for i in range(64)])
        assert bool(torch.isfinite(alone.float()).all()) and float(alone.float().abs().max()) > 0.1
        for M in RI.EVERY_M:
            _same(_gate(ops, x[:M], args), alone[:M], f"gate {lname} {I}x{K} M={M}")
        for M in PERM_MS:
            _same(_gate(ops, xp[:M].contiguous(), args), alone[PERM][:M], f"gate {lname} {I}x{K} permuted rows, M={M}")
        for M in FILL_MS:
            for parity in (1, 0):
                keep = idx[:M] % 2 != parity
                for fname, v in (("large", 1e30), ("nan", float("nan"))):
                    xf = torch.full((M, K), v, dtype=torch.bfloat16, device=DEV)
                    xf[keep] = x[:M][keep]
                    _same(_gate(ops, xf, args)[keep], alone[:M][keep], f"gate {lname} {I}x{K} M={M}, rows of parity {parity} filled with {fname}")
        outs.append(alone)
    assert torch.equal(_bits(outs[0]), _bits(outs[1]))                                  # one result, either layout


# ================================================================================================ values, on exact sums
@pytest.mark.parametrize("N,K", RI.LINEAR_7B)
def test_7b_shapes_are_exact_on_the_exact_designs(N, K):
    ops = _ops()
    for unit in DX.X_UNITS:
        x, w, b, r = DX.make_x(64, K, device=DEV, unit=unit), DX.make_w(N, K, device=DEV), DX.make_bias(N, device=DEV), DX.make_residual(64, N, device=DEV)
        S = DX.exact_product(x, w)
        for name, bias, res in MODES:
            want = DX.expected(x, w, b if bias else None, r if res else None, S=S)
            got = _run(ops, x, w, b if bias else None, r if res else None)
            n, first = DX.mismatches(got, want)
            TOTAL["elements"] += got.numel()
            TOTAL["mismatches"] += n
            assert n == 0, f"{N}x{K} x/{unit} M=64 {name}: {n} bf16 patterns differ from the once-rounded exact sum, first at {first}"
        if (N, K) == (4096, 11008):
            want = DX.expected(x, w, b, r, S=S)
            for M in RI.EVERY_M:
                n, first = DX.mismatches(_run(ops, x[:M], w, b, r[:M]), want[:M])
                TOTAL["elements"] += M * N
                TOTAL["mismatches"] += n
                assert n == 0, f"{N}x{K} x/{unit} M={M} bias+residual: {n} bf16 patterns differ, first at {first}"


@pytest.mark.parametrize("I,K", GATES)
def test_7b_gate_is_exact_on_the_exact_designs(I, K):
    """z1, z2 are exact sums rounded once; the gate on them is the gate kernel's own arithmetic (evo_gelu_gate_bf16), inside the gate bound."""
    ops = _ops()
    w12 = DX.make_gate_weights(I, K, device=DEV)
    layouts = _gate_layouts(ops, w12)
    for unit in DX.X_UNITS:
        x = DX.make_x(64, K, device=DEV, unit=unit)
        g = DX.gate_reference(DX.exact_product(x, w12), I)
        want = ops.gelu_gate(g)
        for lname, args in layouts:
            got = _gate(ops, x, args)
            _, idx, outside = RL.gelu_gate_check(got, g)
            assert not bool(outside.any()), f"gate {lname} {I}x{K} x/{unit} M=64: {int(outside.sum())} elements outside the gate bound (first {idx})"
            n, first = DX.mismatches(got, want)
            TOTAL["elements"] += got.numel()
            TOTAL["mismatches"] += n
            assert n == 0, f"gate {lname} {I}x{K} x/{unit} M=64: {n} bf16 patterns differ from gelu_gate on the exact sums, first at {first}"


# ================================================================================================ which route ran
@pytest.mark.parametrize("N,K", SHAPES)
def test_the_route_is_read_off_a_nan_filled_workspace(N, K):
    """A caller-owned workspace of 8 M N NaN floats: slab s [M, N] is overwritten iff the launch had a slice s.  The count is the restated
    rule's (tests/rowinv_ref.py), the same at M = 1 and M = 64, and 0 on the wide launches."""
    ops = _ops()
    x, w, b, r = _data(N, K)
    want = RI.rowinv_slices(N, K)
    assert (want == 0) == (N >= RI.WIDE_N)
    for M in (1, 64):
        ws = torch.full((8, M, N), float("nan"), dtype=torch.float32, device=DEV)
        y = torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
        TOTAL["launches"] += 1
        rc = ops.lib.evo_linear_rowinv_bf16(x.data_ptr(), w.data_ptr(), None, None, y.data_ptr(), M, N, K, ws.data_ptr(), ws.numel() * 4, None)
        torch.cuda.synchronize()
        assert rc == 0
        nan = torch.isnan(ws).flatten(1)
        written, untouched = (~nan).all(1), nan.all(1)
        assert bool((written | untouched).all()), f"{N}x{K} M={M}: a slab is partly written"
        assert written.tolist() == [s < want for s in range(8)], f"{N}x{K} M={M}: slabs written {written.tolist()}, the rule says {want} slices"
        _same(y, _alone(ops, N, K, 0)[:M], f"{N}x{K} M={M} through the C entry")


# ================================================================================================ teeth
@pytest.mark.parametrize("N,K", RI.LINEAR_7B + [(2 * RI.GATE_7B[0], RI.GATE_7B[1])])
def test_default_routing_sees_the_row_count_on_this_data(N, K):
    """The DEFAULT entry on the same data: some row differs between its one-row call and some M-row call -- this shape's data can see a
    summation order, so the equalities above are not vacuous."""
    ops = _ops()
    x, w = (_data(N, K)[0], _data(N, K)[1]) if (N, K) in RI.LINEAR_7B else _gate_data(N // 2, K)
    alone = torch.cat([ops.linear(x[i:i + 1], w) for i in range(64)])
    found = None
    for M in range(2, 65):
        ne = (_bits(ops.linear(x[:M], w)) != _bits(alone[:M])).any(1)
        if bool(ne.any()):
            found = (int(ne.nonzero()[0]), M, int(ne.sum()))
            break
    print(f"[rowinv rows teeth] default linear {N}x{K}: " + (f"row {found[0]} differs between M = 1 and M = {found[1]} ({found[2]} of {found[1]} rows do)"
                                                                 if found else "no row differs at any M"))
    assert found is not None, f"{N}x{K}: the default entry is row-invariant on this data -- the data cannot see a summation order"


def test_zz_totals():
    """The module's totals (tests/PARITY_batch_invariant.md section 2 is filled from this line)."""
    dt = time.time() - TOTAL["t0"] if TOTAL["t0"] else 0.0
    print(f"[rowinv rows total] launches {TOTAL['launches']}, elements compared {TOTAL['elements']}, mismatching {TOTAL['mismatches']}; "
          f"wall time since the first test {dt:.1f} s")
    assert TOTAL["mismatches"] == 0
