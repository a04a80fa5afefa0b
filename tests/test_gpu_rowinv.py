"""GPU (-m gpu): the row-invariant dense launches of csrc/gemv_inv.hip (evo_linear_rowinv_bf16, evo_mlp_gate_rowinv_bf16; DESIGN.md
section 25) -- row i of an M-row call is bit for bit the one-row call on row i, for every M from 1 to 64 and whatever the other rows hold.

One shape per route of the dispatch, at the smallest N and K that take it (the dispatch is a function of (N, K) alone):
    N >= 8192, 2 / 4 waves per workgroup          (8192, 256), (16384, 256)         [3 waves: the 7B shape 12288 x 4096]
    N < 8192, split over K, 4 waves               (2048, 512): 2 slices of one 256-k unit
                                                  (4096, 1792): 7 units over 4 slices (1, 2, 2, 2) -- an odd number of units, as l3's
                                                  11,008 = 43 x 256; cut in chunks of 4 MFMA steps it would fall elsewhere from 33 rows up
    N < 2048, split over K, 2 waves               (512, 512)
    gate                                          I = 64, K = 512, both weight layouts
N(0, 1) data, for which the order of a sum over K shows in the bits (test_default_routing_is_not_row_invariant proves it on the default
entry); the exact designs of tests/dense_exact.py pin the values themselves; both entries run inside the poisoned arena (tests/arena.py)."""
import pytest
import torch

import dense_exact as DX
import rowlocal_ref as RL
from test_gpu_arena import _run as run_arena, covers, gen, rnd

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SHAPES = [(8192, 256), (16384, 256), (2048, 512), (4096, 1792), (512, 512)]
GATE_SHAPES = [(64, 512)]
MS = [1, 2, 4, 5, 8, 9, 16, 17, 32, 33, 48, 49, 64]
MODES = [("plain", False, False), ("bias", True, False), ("residual", False, True), ("bias+residual", True, True)]
EXACT_MS = [1, 5, 17, 64]
SHAPES_7B = [(12288, 4096), (4096, 4096), (4096, 11008), (512, 4096)]
_DATA = {}


def _ops():
    from evo_amd.ops import default_ops
    ops = default_ops()
    assert ops.supports("row_invariant")
    return ops


def _randn(*shape, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return torch.randn(*shape, generator=g, device=DEV, dtype=torch.float32).to(torch.bfloat16)


def _data(N, K):
    """x [64, K], w [N, K], bias [N], residual [64, N]: N(0, 1), made once per shape and never modified."""
    if (N, K) not in _DATA:
        _DATA[(N, K)] = (_randn(64, K, seed=1), _randn(N, K, seed=2), _randn(N, seed=3), _randn(64, N, seed=4))
    return _DATA[(N, K)]


def _run(ops, x, w, b, r):
    return ops.linear_residual_rowinv_(r.clone(), x, w, bias=b) if r is not None else ops.linear_rowinv(x, w, b)


def _rows_of(M):
    return sorted({0, M // 2, M - 1})


def _fills(M, K, N):
    """The rows that are NOT under test: once large finite values, once NaN (x and residual alike)."""
    for name, v in (("large", 1e30), ("nan", float("nan"))):
        yield name, torch.full((M, K), v, dtype=torch.bfloat16, device=DEV), torch.full((M, N), v, dtype=torch.bfloat16, device=DEV)


@pytest.mark.parametrize("N,K", SHAPES)
def test_linear_rows_do_not_see_each_other(N, K):
    ops = _ops()
    x, w, b, r = _data(N, K)
    for name, bias, res in MODES:
        bb = b if bias else None
        alone = torch.cat([_run(ops, x[i:i + 1], w, bb, r[i:i + 1] if res else None) for i in range(64)])      # the M = 1 results, once
        assert bool(torch.isfinite(alone.float()).all())
        for M in MS:
            rows = _rows_of(M)
            for fname, xf, rf in _fills(M, K, N):
                xf[rows], rf[rows] = x[rows], r[rows]
                got = _run(ops, xf, w, bb, rf if res else None)
                for i in rows:
                    assert torch.equal(got[i], alone[i]), f"{N}x{K} {name} M={M} row {i} ({fname} neighbours) differs from the one-row call"


@pytest.mark.parametrize("I,K", GATE_SHAPES)
def test_gate_rows_do_not_see_each_other(I, K):
    ops = _ops()
    x, w12 = _randn(64, K, seed=5), (_randn(2 * I, K, seed=6).float() * K ** -0.5).to(torch.bfloat16)
    for lname, args in (("plain", (w12, None)), ("grouped", (None, ops.pack_gate_weights(w12)))):
        alone = torch.cat([ops.mlp_gate_rowinv(x[i:i + 1], *args) for i in range(64)])
        assert bool(torch.isfinite(alone.float()).all())
        for M in MS:
            rows = _rows_of(M)
            for fname, xf, _ in _fills(M, K, 1):
                xf[rows] = x[rows]
                got = ops.mlp_gate_rowinv(xf, *args)
                for i in rows:
                    assert torch.equal(got[i], alone[i]), f"gate {lname} {I}x{K} M={M} row {i} ({fname} neighbours) differs from the one-row call"
    assert torch.equal(ops.mlp_gate_rowinv(x, w12), ops.mlp_gate_rowinv(x, None, ops.pack_gate_weights(w12)))      # one result, either layout


@pytest.mark.parametrize("N,K", SHAPES)
def test_linear_is_exact_on_the_exact_designs(N, K):
    ops = _ops()
    for unit in DX.X_UNITS:
        x, w, b, r = DX.make_x(64, K, device=DEV, unit=unit), DX.make_w(N, K, device=DEV), DX.make_bias(N, device=DEV), DX.make_residual(64, N, device=DEV)
        S = DX.exact_product(x, w)
        for M in EXACT_MS:
            for name, bias, res in MODES:
                want = DX.expected(x[:M], w, b if bias else None, r[:M] if res else None, S=S[:M])
                got = _run(ops, x[:M], w, b if bias else None, r[:M] if res else None)
                n, first = DX.mismatches(got, want)
                assert n == 0, f"{N}x{K} x/{unit} M={M} {name}: {n} bf16 patterns differ, first at {first}"


@pytest.mark.parametrize("I,K", GATE_SHAPES + [(1408, 4096)])
def test_gate_is_exact_on_the_exact_designs(I, K):
    """z1, z2 are exact sums rounded once; the gate on them is the gate kernel's own arithmetic (evo_gelu_gate_bf16), inside the gate bound."""
    ops = _ops()
    x, w12 = DX.make_x(64, K, device=DEV, unit=16), DX.make_gate_weights(I, K, device=DEV)
    S = DX.exact_product(x, w12)
    w12g = ops.pack_gate_weights(w12)
    for M in EXACT_MS:
        g = DX.gate_reference(S[:M], I)
        want = ops.gelu_gate(g)
        for lname, args in (("plain", (w12, None)), ("grouped", (None, w12g))):
            got = ops.mlp_gate_rowinv(x[:M], *args)
            _, idx, outside = RL.gelu_gate_check(got, g)
            assert not bool(outside.any()), f"gate {lname} {I}x{K} M={M}: {int(outside.sum())} elements outside the gate bound (first {idx})"
            n, first = DX.mismatches(got, want)
            assert n == 0, f"gate {lname} {I}x{K} M={M}: {n} bf16 patterns differ from gelu_gate on the exact sums, first at {first}"


def test_default_routing_is_not_row_invariant():
    """Teeth: on the same N(0, 1) data the default entry's row 0 differs between its M = 1 and M = 5 results on at least one shape (dot2
    against MFMA: another order over K) -- the data can see what the row-invariant entry removes."""
    ops = _ops()
    differs = {}
    for N, K in SHAPES:
        x, w, b, r = _data(N, K)
        differs[(N, K)] = not torch.equal(ops.linear(x[:1], w)[0], ops.linear(x[:5], w)[0])
        assert torch.equal(ops.linear_rowinv(x[:1], w)[0], ops.linear_rowinv(x[:5], w)[0])
    print(f"[rowinv teeth] default M = 1 vs M = 5, row 0 differs: {differs}")
    assert any(differs.values()), differs


def test_7b_shapes():
    """The 7B step's five layers once each at M = 1 and M = 33: row 0 is the same bits, and the values are the dense layer's."""
    ops = _ops()
    for N, K in SHAPES_7B:
        x, w = _randn(33, K, seed=7), (_randn(N, K, seed=8).float() * K ** -0.5).to(torch.bfloat16)
        one, many = ops.linear_rowinv(x[:1], w), ops.linear_rowinv(x, w)
        assert torch.equal(many[0], one[0]), (N, K)
        ref = x.double() @ w.double().t()
        assert float((many.double() - ref).norm() / ref.norm()) < 4e-3, (N, K)          # one bf16 rounding: 2^-9 per element at the worst
    I, K = 11008, 4096
    x, w12 = _randn(33, K, seed=9), (_randn(2 * I, K, seed=10).float() * K ** -0.5).to(torch.bfloat16)
    one, many = ops.mlp_gate_rowinv(x[:1], w12), ops.mlp_gate_rowinv(x, w12)
    assert torch.equal(many[0], one[0])
    assert torch.equal(many, ops.gelu_gate(ops.linear_rowinv(x, w12)))                   # the gate on the dense layer's rounded outputs


def test_shapes_outside_the_contract_are_errors():
    ops = _ops()
    x = _randn(2, 264, seed=11)
    with pytest.raises(RuntimeError):
        ops.linear_rowinv(x, _randn(64, 264, seed=12))                                    # K % 256
    with pytest.raises(RuntimeError):
        ops.linear_rowinv(_randn(2, 256, seed=13), _randn(40, 256, seed=14))              # N % 64
    with pytest.raises(RuntimeError):
        ops.linear_rowinv(_randn(65, 256, seed=15), _randn(64, 256, seed=16))             # 65 rows
    with pytest.raises(RuntimeError):
        ops.mlp_gate_rowinv(_randn(2, 256, seed=17), _randn(2 * 40, 256, seed=18))        # I % 32
    lib = ops.lib
    xx, ww, yy = _randn(2, 256, seed=19), _randn(64, 256, seed=20), torch.empty(2, 64, dtype=torch.bfloat16, device=DEV)
    assert lib.evo_linear_rowinv_bf16(xx.data_ptr(), ww.data_ptr(), None, None, yy.data_ptr(), 2, 64, 256, None, 0, None) == -1      # no workspace
    assert lib.evo_linear_rowinv_bf16(xx.data_ptr(), ww.data_ptr(), None, None, yy.data_ptr(), 2, 64, 264, None, 0, None) == -1
    assert lib.evo_mlp_gate_rowinv_bf16(xx.data_ptr(), ww.data_ptr(), yy.data_ptr(), 65, 32, 256, 0, None) == -1


# ================================================================================================ the arena
@covers("evo_linear_rowinv_bf16")
@pytest.mark.parametrize("M,N,K", [(1, 8192, 256), (33, 8256, 512), (5, 2048, 512), (64, 4096, 1792), (17, 512, 512), (49, 64, 256)])
def test_arena_linear(M, N, K):
    """Every route, a ragged last workgroup of the wide one (8256 = 129 n tiles of 64 rows), the smallest narrow layer; the workspace of
    the K slices is carved too.  Two rows behind M keep their bits."""
    ops = _ops()
    inp = {"x": rnd((M, K), gen(M)), "w": rnd((N, K), gen(1), K ** -0.5), "b": rnd((N,), gen(2)), "res": rnd((M + 2, N), gen(3))}
    run_arena(lambda x, w, b, res: ops.linear_residual_rowinv_(res[:M], x, w, bias=b), inp, inout=["res"], expect=["evo_linear_rowinv_bf16"])
    run_arena(lambda x, w, b, res: ops.linear_rowinv(x, w), inp, expect=["evo_linear_rowinv_bf16"])


@covers("evo_mlp_gate_rowinv_bf16")
@pytest.mark.parametrize("M,I,K,grouped", [(1, 32, 256, False), (17, 64, 512, True), (40, 96, 256, False), (64, 1408, 4096, True)])
def test_arena_gate(M, I, K, grouped):
    ops = _ops()
    inp = {"x": rnd((M, K), gen(M)), "w12": rnd((2 * I, K), gen(1), K ** -0.5)}
    run_arena(lambda x, w12: ops.mlp_gate_rowinv(x, None, w12) if grouped else ops.mlp_gate_rowinv(x, w12), inp, expect=["evo_mlp_gate_rowinv_bf16"])
