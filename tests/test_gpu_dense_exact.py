"""GPU (-m gpu): the dense layers (csrc/gemm.hip, csrc/gemv.hip) on EXACT sums -- every launch form, one rounding.

The operands are small integers (tests/dense_exact.py; tests/test_dense_exact_host.py pins the invariants): every fp32 partial sum of
x w^T + bias + residual is exact in any order, so the expected output is ONE bf16 bit pattern per element -- the round-to-nearest-even
rounding of the exact fp64 sum, 15-22 % of the elements being exact ties and 16-70 % not representable.  Comparison is `torch.equal` on the
int16 views; no element is left out and there is no tolerance.  A truncating pack, a bias or residual added after a rounding, a partial
sum that crosses LDS or the workspace in bf16, a dropped or duplicated k element, a wrong row or column: each changes bits, and the
message names the first (row, column).  The gated launches are judged by row 24b's per-element bound (rowlocal_ref.gelu_gate_bound) on
g = [bf16(S1) | bf16(S2)] of the exact products.  Every launch is issued twice (equal results) and its launch class is asserted through
the launch timer's spans (the SPLITK form through a workspace filled with NaN: the slices it wrote are counted).

The weight-streaming forms run on a SECOND data set as well (ids `sixteenths`: x in multiples of 1/16, still exact -- dense_exact.make_x).
A partial sum of integers below 256 is itself a bf16 number, so on the integer data a partial sum crossing LDS in bf16 shows at K = 4,096
only (0.5 % of the elements; measured on a scratch build: 17 elements of one test); on sixteenths it changes 32-40 % of the elements at
K = 288 and 4,096 alike (tests/test_dense_exact_host.py).

Instantiation -> the test that reaches it (ids abridged):
  gemm_bf16_kernel<BIAS, RES> (K = 64)                         test_persistent_and_tile_per_workgroup[9-256-64 | 300-512-64 | 513-256-64]
  launch_persistent<0, false, 0> (+ BIAS / RES)                test_persistent_and_tile_per_workgroup[K >= 128], test_linear_across_the_sliver_seam
  launch_persistent<0, true, 0>   blocked-y input              test_blocked_input
  launch_persistent<0, false, 1>  sum-of-squares producer      test_sum_of_squares_producer[direct-*]
  launch_persistent<0, true, 1>                                test_sum_of_squares_producer[blocked-*]
  launch_persistent<0, false, 2>  row_scale consumer           test_row_scale_consumer
  launch_persistent<1, false, 0>  gated                        test_gated_launch[plain-*]
  launch_persistent<1, false, 2>                               test_gated_launch[row_scale-*]
  launch_persistent<3, false, 0>  transposed z^T               test_transposed_launch[plain-*]
  launch_persistent<3, false, 2>  (+ row_skip in the tail form) test_transposed_launch[row_scale-*]
  evo_linear_small_m_bf16:
    gemv_kernel<1..8, 4, false>                                test_dot2[37-264] (M 1..8), [12288-4096], [8200-768] (M <= 4)
    gemv_kernel<1..8, 4, true> (SPLIT)                         test_dot2[4095-2056], [4096-10928] (M 1..8), [4096-4096] (M <= 4)
    skinny_mfma_kernel<1..4, 1>                                test_skinny_mfma[37-288], [512-4096]; [8192-288] / [8200-288] at M <= 16;
                                                               test_splitk[4096-512] (must not split)
    skinny_mfma_kernel<2..4, 2>                                test_skinny_mfma[8192-288], [8200-288] from 17 rows
    skinny_nw_kernel<1..4, 2>                                  test_skinny_nw[8200-256], [8200-768]
    skinny_nw_kernel<1..4, 3>                                  test_skinny_nw[12288-4096], [12296-512]
    skinny_nw_kernel<1..4, 4>                                  test_skinny_nw[16384-256]
    skinny_nw_kernel<2..4, 4, SPLITK> + skinny_reduce_kernel   test_splitk (MT 3, 4: M 33, 64; MT 2: M 17, 32 at K >= 8192; 3 / 4 / 8 slices)
  evo_mlp_gate_small_m_bf16:
    gemv_gate_kernel<1..4, false, false> (both layouts)        test_gate_small_m (M <= 4)
    skinny_nw_kernel<1..4, 4, false, GATE> (both layouts)      test_gate_small_m (M 5..8 -> MT 1, 13 -> 1, 17 -> 2, 40 -> 3, 64 -> 4)
  evo_norm_linear_small_m_bf16:
    gemv_norm_kernel<1..8, 4, true>                            test_norm_linear[4104-4096], [12288-4096]
    gemv_norm_kernel<1..4, 4, false>                           test_norm_linear[4104-256], [4104-1024]
  evo_norm_mlp_gate_small_m_bf16:
    gemv_gate_kernel<1..8, true, true>                         test_norm_gate[1408-4096]
    gemv_gate_kernel<1..4, true, false>                        test_norm_gate[64-256], [64-1024]
  evo_hyena_decode_fused_small_m:
    gemv_norm_hyena_kernel<1..8, 1, true>                      test_hyena_decode_fused[4096]   (z_t at every M; the outputs at M = 1, 4, 5, 8)
    gemv_norm_hyena_kernel<1, 1 | 2, 2 | 3, 2 | 4, 1, false>   test_hyena_decode_fused[256], [1024]
"""
import time

import pytest
import torch

import dense_exact as DX
import rowlocal_ref as RL

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = DX.EPS
MODES = [("plain", False, False), ("bias", True, False), ("residual", False, True), ("both", True, True)]
TOTAL = dict(cases=0, elements=0, mismatches=0, gate_cases=0, gate_outside=0, t0=None)


def _ops():
    from evo_amd.ops import default_ops
    if TOTAL["t0"] is None:
        TOTAL["t0"] = time.time()
    return default_ops()


class _Spans:
    """The launch timer's spans of the launches issued inside the block: {span name: launches}."""

    def __init__(self, ops):
        self.ops, self.count = ops, {}

    def __enter__(self):
        from evo_amd.ops import KernelTimer
        self.was = self.ops.timer
        self.ops.timer = KernelTimer()
        return self

    def __exit__(self, *exc):
        self.count = {k: len(v) for k, v in self.ops.timer.pairs.items()}
        self.ops.timer = self.was
        return False


def _exact(got, want, what):
    """Every bf16 bit pattern of `got` equals `want`."""
    n, first = DX.mismatches(got, want)
    TOTAL["cases"] += 1
    TOTAL["elements"] += want.numel()
    TOTAL["mismatches"] += n
    if n:
        r, c = first[0], first[-1]
        pytest.fail(f"{what}: {n} of {want.numel()} bf16 patterns differ, first at {first}: got {float(got[first]):.10g} "
                    f"(0x{int(DX.bits(got)[first]) & 0xffff:04x}), want {float(want[first]):.10g} (0x{int(DX.bits(want)[first]) & 0xffff:04x}) "
                    f"[row {r}, column {c}]", pytrace=False)


def _gate(got, g, what):
    """Every element of the gate output inside rowlocal_ref.gelu_gate_bound of gelu_gate64(g)."""
    worst, idx, outside = RL.gelu_gate_check(got, g)
    TOTAL["gate_cases"] += 1
    TOTAL["gate_outside"] += int(outside.sum())
    assert not bool(outside.any()), f"{what}: {int(outside.sum())} elements outside the gate bound, worst err / bound {worst:.3f} at flat index {idx}"
    return worst


def _report(group, t0, n0, extra=""):
    print(f"[dense_exact {group}] cases {TOTAL['cases'] + TOTAL['gate_cases'] - n0}, mismatching elements {TOTAL['mismatches']}, "
          f"gate elements outside the bound {TOTAL['gate_outside']}{extra}, {time.time() - t0:.1f} s")


def _n0():
    return TOTAL["cases"] + TOTAL["gate_cases"]


def _pad256(v):
    out = torch.ones((v.numel() + 255) // 256 * 256, dtype=torch.float32, device=v.device)
    out[:v.numel()] = v
    return out


def _pack_yblk(ops, y):
    """Row-major y [M, K] -> the blocked layout [ceil(M / 128), K / 16, 128, 16] (pad rows zero)."""
    M, K = y.shape
    nrb = (M + 127) // 128
    pad = torch.zeros(nrb * 128, K, dtype=torch.bfloat16, device=y.device)
    pad[:M] = y
    y_blk = pad.view(nrb, 128, K // 16, 16).permute(0, 2, 1, 3).contiguous()
    assert torch.equal(ops.yblk_to_rows(y_blk, M), y)
    return y_blk


def test_constructors_give_the_same_tensors_on_the_device():
    """The hash is wrapping int64 arithmetic: the operands made on the GPU are the ones tests/test_dense_exact_host.py checked on the CPU."""
    for unit in DX.X_UNITS:
        assert torch.equal(DX.make_x(70, 4096, device=DEV, unit=unit).cpu(), DX.make_x(70, 4096, unit=unit))
    assert torch.equal(DX.make_w(300, 11008, device=DEV).cpu(), DX.make_w(300, 11008))
    assert torch.equal(DX.make_bias(4104, device=DEV).cpu(), DX.make_bias(4104))
    assert torch.equal(DX.make_residual(70, 4095, device=DEV).cpu(), DX.make_residual(70, 4095))
    assert torch.equal(DX.make_gate_weights(64, 264, device=DEV).cpu(), DX.make_gate_weights(64, 264))
    assert torch.equal(DX.make_pow2_rows(300, device=DEV).cpu(), DX.make_pow2_rows(300))
    assert torch.equal(DX.make_sparse_x(70, 192, device=DEV).cpu(), DX.make_sparse_x(70, 192))
    assert torch.equal(DX.make_int_residual(70, 256, device=DEV).cpu(), DX.make_int_residual(70, 256))
    for K in (256, 4096):
        (xg, ag), (xc, ac) = DX.make_norm_rows(8, K, device=DEV), DX.make_norm_rows(8, K)
        assert torch.equal(xg.cpu(), xc) and torch.equal(ag.cpu(), ac)
        assert torch.equal(DX.make_norm_scale(K, device=DEV).cpu(), DX.make_norm_scale(K))


# =============================================================================== the persistent kernel and its tile-per-workgroup sibling
@pytest.mark.parametrize("M,N,K", DX.PERSISTENT)
def test_persistent_and_tile_per_workgroup(M, N, K):
    """evo_linear_mfma_bf16 x {plain, bias, residual, both}; the residual buffer carries 64 rows behind M, which keep their bits."""
    ops = _ops()
    t0, n0 = time.time(), _n0()
    x, w, b = DX.make_x(M, K, device=DEV), DX.make_w(N, K, device=DEV), DX.make_bias(N, device=DEV)
    r = DX.make_residual(M + 64, N, device=DEV)
    S = DX.exact_product(x, w)
    for name, bias, res in MODES:
        want = DX.expected(x, w, b if bias else None, r[:M] if res else None, S=S)

        def run():
            if not res:
                return ops.linear_mfma(x, w, b if bias else None)
            buf = r.clone()
            out = ops.linear_mfma(x, w, b if bias else None, buf[:M])
            assert out.data_ptr() == buf.data_ptr()
            assert torch.equal(DX.bits(buf[M:]), DX.bits(r[M:])), "rows behind M were written"
            return buf[:M]
        with _Spans(ops) as sp:
            got, again = run(), run()
        assert sp.count == {"gemm_mfma": 2}, sp.count
        _exact(got, want, f"linear_mfma {M}x{N}x{K} {name}")
        assert torch.equal(got, again)
    _report(f"persistent {M}x{N}x{K}", t0, n0)


@pytest.mark.parametrize("M,N,K", DX.XBLK)
def test_blocked_input(M, N, K):
    """evo_linear_xblk_mfma_bf16 through linear_residual_yblk_ (residual, residual + bias)."""
    ops = _ops()
    t0, n0 = time.time(), _n0()
    y, w, b, r = DX.make_x(M, K, device=DEV), DX.make_w(N, K, device=DEV), DX.make_bias(N, device=DEV), DX.make_residual(M, N, device=DEV)
    y_blk = _pack_yblk(ops, y)
    S = DX.exact_product(y, w)
    for bias in (False, True):
        want = DX.expected(y, w, b if bias else None, r, S=S)
        with _Spans(ops) as sp:
            got = ops.linear_residual_yblk_(r.clone(), y_blk, w, bias=b if bias else None)
            again = ops.linear_residual_yblk_(r.clone(), y_blk, w, bias=b if bias else None)
        assert sp.count == {"gemm_mfma": 2}, sp.count
        _exact(got, want, f"blocked input {M}x{N}x{K} bias={bias}")
        assert torch.equal(got, again)
    _report(f"blocked input {M}x{N}x{K}", t0, n0)


@pytest.mark.parametrize("M,I,K", DX.GATED)
@pytest.mark.parametrize("form", ["plain", "row_scale"])
def test_gated_launch(form, M, I, K):
    """evo_mlp_gate_mfma(_nf)_bf16: GELU x gate in the epilogue on z1 = bf16(S1), z2 = bf16(S2) (row_scale: bf16(2^e S)), row 24b's bound."""
    ops = _ops()
    t0, n0 = time.time(), _n0()
    x, w12 = DX.make_x(M, K, device=DEV), DX.make_gate_weights(I, K, device=DEV)
    w12g = ops.pack_gate_weights(w12)
    S = DX.exact_product(x, w12)
    if form == "plain":
        Mm = M
        g = DX.gate_reference(S, I)
        with _Spans(ops) as sp:
            got, again = ops.mlp_gate(x, w12, w12g=w12g), ops.mlp_gate(x, w12, w12g=w12g)
        assert sp.count == {"gemm_gate": 2}, sp.count
    else:
        Mm = ops._nf_main_rows(M)                                       # (a sliver row behind the last whole tile takes the norm-folding small-M launch: not this epilogue)
        p2 = DX.make_pow2_rows(M, device=DEV)
        g = DX.gate_reference(DX.exact_sum(x, w12, row_scale=p2, S=S), I)[:Mm]
        ones = torch.ones(K, dtype=torch.bfloat16, device=DEV)
        with _Spans(ops) as sp:
            got, again = ops.mlp_gate_rs(x, _pad256(p2), w12g, w12, ones, EPS)[:Mm], ops.mlp_gate_rs(x, _pad256(p2), w12g, w12, ones, EPS)[:Mm]
        assert sp.count.get("gemm_gate") == 2, sp.count
    assert float(g[:, :I].double().std()) > (0.2 if K < 4096 else 1.0)             # u spans the GELU's curved range
    worst = _gate(got, g, f"gated launch {form} {M}x{I}x{K}")
    assert torch.equal(got, again)
    _report(f"gated {form} {M}x{I}x{K}", t0, n0, f", worst err / bound {worst:.3f}")


@pytest.mark.parametrize("B,T,N,K", DX.LINEAR_T)
@pytest.mark.parametrize("form", ["plain", "row_scale"])
def test_transposed_launch(form, B, T, N, K):
    """evo_linear_t_mfma(_nf)_bf16: z^T in blocks of 256 positions, on the plain form (2 x 640: no pad position) and the tail form
    (3 x 1,026: rows of 1,024 positions, row_skip = 2, the tail tokens through the weight-streaming launch into the tail block)."""
    ops = _ops()
    t0, n0 = time.time(), _n0()
    Tm, Tp, Mp, r = ops.zt_layout(B, T)
    assert (r, Tp, Mp) == ((0, 640, 1280) if T == 640 else (2, 1024, 3072))
    M = B * T
    x, w, b = DX.make_x(M, K, device=DEV), DX.make_w(N, K, device=DEV), DX.make_bias(N, device=DEV)
    S = DX.exact_product(x, w)
    if form == "plain":
        xp = torch.zeros(Mp + 16, K, dtype=torch.bfloat16, device=DEV)               # rmsnorm_rows' layout, filled by hand
        bb = torch.arange(B, device=DEV)[:, None].expand(B, T).reshape(-1)
        tt = torch.arange(T, device=DEV)[None, :].expand(B, T).reshape(-1)
        rows = torch.where(tt < Tm, bb * Tp + tt, Mp + bb * r + (tt - Tm))
        xp[rows] = x
        for bias in (False, True):
            want = ops.zt_from_rows(DX.expected(x, w, b if bias else None, S=S).view(B, T, N), B, T)
            with _Spans(ops) as sp:
                got, again = ops.linear_t(xp, w, b if bias else None, B, T), ops.linear_t(xp, w, b if bias else None, B, T)
            assert sp.count == ({"gemm_zt": 2, "gemv": 2} if r else {"gemm_zt": 2}), sp.count
            _exact(got, want, f"linear_t {B}x{T}x{N}x{K} bias={bias}")
            assert torch.equal(got, again)
    else:
        assert ops.zt_stream_rows_ok(B, T)
        p2 = DX.make_pow2_rows(M, device=DEV)
        ones = torch.ones(K, dtype=torch.bfloat16, device=DEV)
        for bias in (False, True):
            want = ops.zt_from_rows(DX.expected(x, w, b if bias else None, row_scale=p2, S=S).view(B, T, N), B, T)[:Mp // 256]
            with _Spans(ops) as sp:                                                    # (tail=False: the main area; the tail tokens' norm-folding launch is test_norm_linear's)
                got = ops.linear_t_rs(x, _pad256(p2), w, b if bias else None, w, ones, EPS, B, T, tail=False)
                again = ops.linear_t_rs(x, _pad256(p2), w, b if bias else None, w, ones, EPS, B, T, tail=False)
            assert sp.count == {"gemm_zt": 2}, sp.count
            _exact(got, want, f"linear_t_rs {B}x{T}x{N}x{K} bias={bias}")
            assert torch.equal(got, again)
    _report(f"transposed {form} {B}x{T}x{N}x{K}", t0, n0)


@pytest.mark.parametrize("M,N,K", DX.ROW_SCALE)
def test_row_scale_consumer(M, N, K):
    """evo_linear_mfma_nf_bf16 (row_scale): factors 2^-3 .. 2^3, different per row, multiply the accumulators BEFORE the bias -- exact, so
    the result is compared with expected() itself (which row got which factor, where the bias is added), not with the plain launch."""
    ops = _ops()
    t0, n0 = time.time(), _n0()
    x, w, b = DX.make_x(M, K, device=DEV), DX.make_w(N, K, device=DEV), DX.make_bias(N, device=DEV)
    p2 = DX.make_pow2_rows(M, device=DEV)
    Mm = ops._nf_main_rows(M)
    ones = torch.ones(K, dtype=torch.bfloat16, device=DEV)
    S = DX.exact_product(x, w)
    for bias in (False, True):
        want = DX.expected(x, w, b if bias else None, row_scale=p2, S=S)[:Mm]
        with _Spans(ops) as sp:
            got, again = ops.linear_rs(x, _pad256(p2), w, b if bias else None, w, ones, EPS)[:Mm], ops.linear_rs(x, _pad256(p2), w, b if bias else None, w, ones, EPS)[:Mm]
        assert sp.count.get("gemm_mfma") == 2, sp.count
        _exact(got.contiguous(), want.contiguous(), f"row_scale consumer {M}x{N}x{K} bias={bias}")
        assert torch.equal(got, again)
    _report(f"row_scale {M}x{N}x{K}", t0, n0)


@pytest.mark.parametrize("M,N,K", DX.SUMSQ)
@pytest.mark.parametrize("src", ["direct", "blocked"])
def test_sum_of_squares_producer(src, M, N, K):
    """evo_linear(_xblk)_mfma_nf_bf16 (sumsq): x rows of 8 nonzeros of +-1 and an integer residual, so the stored rows are integers with
    |y| <= 24 and a 128-column strip's sum of squares is an integer <= 73,728: the sumsq buffer must EQUAL the fp64 sums in every
    (strip, main row) entry, the stored rows their exact values, and rms_finalize's factor stays inside row 11a's 2e-6."""
    ops = _ops()
    t0, n0 = time.time(), _n0()
    x, w, r = DX.make_sparse_x(M, K, device=DEV), DX.make_w(N, K, device=DEV), DX.make_int_residual(M, N, device=DEV)
    want = DX.expected(x, w, None, r)
    assert float(want.double().abs().max()) <= 24
    xb = _pack_yblk(ops, x) if src == "blocked" else None
    seen = []
    finalize = ops.rms_finalize

    def spy(ss, xx, m_main, eps):
        seen.append((ss, m_main))
        return finalize(ss, xx, m_main, eps)
    ops.rms_finalize = spy
    try:
        outs = []
        for _ in range(2):
            got = r.clone()
            with _Spans(ops) as sp:
                rstd = ops.linear_residual_stats_(got, x, w, None, EPS) if src == "direct" else ops.linear_residual_yblk_stats_(got, xb, w, None, EPS)
            assert sp.count.get("gemm_mfma", 0) >= 1 and sp.count.get("rms_finalize") == 1, sp.count
            outs.append((got, rstd))
    finally:
        del ops.rms_finalize
    (got, rstd), (again, rstd2) = outs
    _exact(got, want, f"sumsq producer {src} {M}x{N}x{K}: stored rows")
    assert torch.equal(got, again) and torch.equal(rstd[:M], rstd2[:M])
    ss, Mm = seen[0]
    assert Mm == (ops._nf_main_rows(M) if src == "direct" else M // 256 * 256) and ss.shape[0] == N // 128
    ss_want = want[:Mm].double().pow(2).view(Mm, N // 128, 128).sum(-1).t()
    assert float(ss_want.max()) <= 73728
    bad = ss[:, :Mm].double() != ss_want
    TOTAL["cases"] += 1
    TOTAL["elements"] += ss_want.numel()
    TOTAL["mismatches"] += int(bad.sum())
    assert not bool(bad.any()), f"{int(bad.sum())} of {bad.numel()} strip sums differ, first (strip, row) {bad.nonzero()[0].tolist()}"
    ref = 1.0 / (want.double().pow(2).sum(-1).sqrt() * N ** -0.5 + EPS)
    rel = float(((rstd[:M].double() - ref).abs() / ref).max())
    assert rel < 2e-6, rel
    _report(f"sumsq {src} {M}x{N}x{K}", t0, n0, f", rstd rel err {rel:.2e}")


@pytest.mark.parametrize("M,N,K", DX.SEAM)
def test_linear_across_the_sliver_seam(M, N, K):
    """HipOps.linear / linear_residual_ (all_gemm_mfma): 1 and 16 rows behind the last whole tile go to the weight-streaming kernel, 17 stay."""
    ops = _ops()
    assert ops.all_gemm_mfma
    t0, n0 = time.time(), _n0()
    x, w, b, r = DX.make_x(M, K, device=DEV), DX.make_w(N, K, device=DEV), DX.make_bias(N, device=DEV), DX.make_residual(M, N, device=DEV)
    S = DX.exact_product(x, w)
    sliver = M % 256 if M % 256 <= 16 else 0
    for name, bias, res in MODES:
        want = DX.expected(x, w, b if bias else None, r if res else None, S=S)

        def run():
            return ops.linear_residual_(r.clone(), x, w, bias=b if bias else None) if res else ops.linear(x, w, b if bias else None)
        with _Spans(ops) as sp:
            got, again = run(), run()
        assert sp.count == ({"gemm_mfma": 2, "gemv": 2} if sliver else {"gemm_mfma": 2}), sp.count
        _exact(got, want, f"linear across the seam {M}x{N}x{K} {name}")
        assert torch.equal(got, again)
    _report(f"seam {M}x{N}x{K}", t0, n0)


# =============================================================================== the weight-streaming forms
UNITS = pytest.mark.parametrize("unit", DX.X_UNITS, ids=["ints", "sixteenths"])     # x in integers (the data of every test here) / in multiples of 1/16


def _small_m_group(ops, N, K, Ms, group, unit):
    """evo_linear_small_m_bf16 through HipOps.linear / linear_residual_ for every M of Ms x {plain, bias, residual, both}."""
    t0, n0 = time.time(), _n0()
    Mx = max(Ms)
    group = f"{group} x/{unit}"
    x, w, b, r = DX.make_x(Mx, K, device=DEV, unit=unit), DX.make_w(N, K, device=DEV), DX.make_bias(N, device=DEV), DX.make_residual(Mx, N, device=DEV)
    S = DX.exact_product(x, w)
    for M in Ms:
        xm = x[:M]
        assert ops._use_small_m(xm, w)
        for name, bias, res in MODES:
            want = DX.expected(xm, w, b if bias else None, r[:M] if res else None, S=S[:M])

            def run():
                return ops.linear_residual_(r[:M].clone(), xm, w, bias=b if bias else None) if res else ops.linear(xm, w, b if bias else None)
            with _Spans(ops) as sp:
                got, again = run(), run()
            assert sp.count == {"gemv": 2}, sp.count
            _exact(got, want, f"{group} M={M} N={N} K={K} {name}")
            assert torch.equal(got, again)
    _report(f"{group} {N}x{K}", t0, n0)


@UNITS
@pytest.mark.parametrize("N,K", DX.DOT2 + DX.DOT2_LE4)
def test_dot2(N, K, unit):
    """gemv_kernel<M, 4, SPLIT>: every M in 1 .. 8 where K % 32 != 0 keeps 5-8 rows on it, M <= 4 elsewhere."""
    Ms = range(1, 9) if K % 32 else range(1, 5)
    _small_m_group(_ops(), N, K, list(Ms), "dot2", unit)


@UNITS
@pytest.mark.parametrize("N,K", DX.SKINNY_MFMA)
def test_skinny_mfma(N, K, unit):
    """skinny_mfma_kernel<MT, NT>: the k-split MFMA form (eight waves' partial tiles meet in LDS in fp32)."""
    _small_m_group(_ops(), N, K, DX.SKINNY_M, "skinny_mfma", unit)


@UNITS
@pytest.mark.parametrize("N,K", DX.SKINNY_NW)
def test_skinny_nw(N, K, unit):
    """skinny_nw_kernel<MT, WAVES>: the n-split MFMA form, 2 / 3 / 4 waves, a ragged last n tile, one / three / sixteen chunks."""
    _small_m_group(_ops(), N, K, DX.SKINNY_M, "skinny_nw", unit)


@UNITS
@pytest.mark.parametrize("Ms,N,K,slices", DX.SPLITK)
def test_splitk(Ms, N, K, slices, unit):
    """skinny_nw_kernel<MT, 4, SPLITK> + skinny_reduce_kernel.  The launch timer gives every weight-streaming launch the one span
    `gemv`, so the launch CLASS is read off the workspace: the second launch gets one filled with NaN, and the [M, N] slabs the kernel
    overwrote are counted -- `slices` of them whole, none in part (0: the shape must NOT split)."""
    ops = _ops()
    t0, n0 = time.time(), _n0()
    Mx = max(Ms)
    x, w, b, r = DX.make_x(Mx, K, device=DEV, unit=unit), DX.make_w(N, K, device=DEV), DX.make_bias(N, device=DEV), DX.make_residual(Mx, N, device=DEV)
    S = DX.exact_product(x, w)
    for M in Ms:
        xm = x[:M].contiguous()
        for name, bias, res in MODES:
            want = DX.expected(xm, w, b if bias else None, r[:M] if res else None, S=S[:M])
            with _Spans(ops) as sp:
                got = ops.linear_residual_(r[:M].clone(), xm, w, bias=b if bias else None) if res else ops.linear(xm, w, b if bias else None)
                ws = torch.full((8, M * N), float("nan"), dtype=torch.float32, device=DEV)
                again = r[:M].clone() if res else torch.empty(M, N, dtype=torch.bfloat16, device=DEV)
                ops._launch("gemv", "evo_linear_small_m_bf16", xm.data_ptr(), w.data_ptr(), b.data_ptr() if bias else None,
                            again.data_ptr() if res else None, again.data_ptr(), M, N, K, ws.data_ptr(), ws.numel() * 4)
            assert sp.count == {"gemv": 2}, sp.count
            written = (~torch.isnan(ws)).sum(-1)
            assert sorted(written.tolist(), reverse=True) == [M * N] * slices + [0] * (8 - slices), f"M={M}: workspace slabs written {written.tolist()}, want {slices} whole"
            _exact(got, want, f"splitk M={M} N={N} K={K} {name}")
            assert torch.equal(got, again)
    _report(f"splitk x/{unit} {N}x{K} ({slices} slices)", t0, n0)


# =============================================================================== the gate at small M
def _gate_cases(ops, xm, w12, S12, what, **kw):
    """mlp_gate on the plain and (I % 32 == 0) the grouped weight layout, each twice; -> worst err / bound."""
    I = w12.shape[0] // 2
    g = DX.gate_reference(S12, I)
    worst = 0.0
    layouts = [("plain", (xm, w12), {})] + ([("grouped", (xm, None), dict(w12g=ops.pack_gate_weights(w12)))] if I % 32 == 0 else [])
    for lname, args, lkw in layouts:
        with _Spans(ops) as sp:
            got, again = ops.mlp_gate(*args, **kw, **lkw), ops.mlp_gate(*args, **kw, **lkw)
        assert sp.count == {"gemv_gate": 2}, (what, lname, sp.count)
        worst = max(worst, _gate(got, g, f"{what} {lname}"))
        assert torch.equal(got, again)
    return worst


@UNITS
@pytest.mark.parametrize("I,K", DX.GATE_SMALL)
def test_gate_small_m(I, K, unit):
    """evo_mlp_gate_small_m_bf16: dot2 launch up to 4 rows, the MFMA form with the gate in its epilogue from 5 (z2 crosses LDS in fp32)."""
    ops = _ops()
    assert ops.gate_small_m_mfma
    t0, n0 = time.time(), _n0()
    Ms = [m for m in DX.GATE_SMALL_M if m <= 4] if K % 256 else DX.GATE_SMALL_M
    x, w12 = DX.make_x(max(Ms), K, device=DEV, unit=unit), DX.make_gate_weights(I, K, device=DEV)
    S = DX.exact_product(x, w12)
    worst = max(_gate_cases(ops, x[:M], w12, S[:M], f"mlp_gate x/{unit} M={M} I={I} K={K}") for M in Ms)
    _report(f"gate small M x/{unit} {I}x{K}", t0, n0, f", worst err / bound {worst:.3f}")


# =============================================================================== a norm in front
def _norm_rows(ops, M, K):
    """make_norm_rows, and FIRST: evo_rmsnorm_bf16 returns exactly the predicted integer rows (else the group stops here)."""
    x, a = DX.make_norm_rows(M, K, device=DEV)
    g = DX.make_norm_scale(K, device=DEV)
    xn = DX.norm_rows_expected(x, g, a)
    got = ops.rmsnorm(x.clone(), None, g, EPS)
    n, first = DX.mismatches(got, xn)
    assert n == 0, f"rmsnorm_kernel is not exact on the designed rows: {n} elements, first {first}: got {float(got[first])} want {float(xn[first])} (a = {a.tolist()})"
    return x, g, xn


@pytest.mark.parametrize("N,K", DX.NORM_LINEAR)
def test_norm_linear(N, K):
    ops = _ops()
    t0, n0 = time.time(), _n0()
    Ms = range(1, 9) if K == 4096 else range(1, 5)
    x, g, xn = _norm_rows(ops, 8, K)
    w, b = DX.make_w(N, K, device=DEV), DX.make_bias(N, device=DEV)
    S = DX.exact_product(xn, w)
    for M in Ms:
        for bias in (False, True):
            want = DX.expected(xn[:M], w, b if bias else None, S=S[:M])
            with _Spans(ops) as sp:
                got, again = ops.norm_linear(x[:M], g, EPS, w, b if bias else None), ops.norm_linear(x[:M], g, EPS, w, b if bias else None)
            assert sp.count == {"gemv_norm": 2}, sp.count
            _exact(got, want, f"norm_linear M={M} N={N} K={K} bias={bias}")
            assert torch.equal(got, again)
    _report(f"norm_linear {N}x{K}", t0, n0)


@pytest.mark.parametrize("I,K", DX.NORM_GATE)
def test_norm_gate(I, K):
    ops = _ops()
    t0, n0 = time.time(), _n0()
    Ms = range(1, 9) if K == 4096 else range(1, 5)
    x, g, xn = _norm_rows(ops, 8, K)
    w12 = DX.make_gate_weights(I, K, device=DEV)
    S = DX.exact_product(xn, w12)
    worst = max(_gate_cases(ops, x[:M], w12, S[:M], f"mlp_gate(norm) M={M} I={I} K={K}", norm_scale=g, eps=EPS) for M in Ms)
    _report(f"norm gate {I}x{K}", t0, n0, f", worst err / bound {worst:.3f}")


@pytest.mark.parametrize("D,Ms", DX.HYENA_FUSED)
def test_hyena_decode_fused(D, Ms):
    """evo_hyena_decode_fused_small_m from zero FIR / modal states: the z_t the launch computed (norm -> projection + bias), read back from
    fir_state's newest column, must equal expected() bit for bit; the outputs stay under row 22d's bound (2^-8 |ref| + 2e-3 of the
    channel's largest + 1e-4 of its terms) against the fp64 operator on exactly those z rows.  The launch's FIR / modal / gate tail is
    held bit for bit, from non-zero states, in tests/test_gpu_hyena_fused_exact.py (PARITY row 9e)."""
    import math
    from gpu_ref64 import gpu_fft_hyena
    ops = _ops()
    t0, n0 = time.time(), _n0()
    H = D // 128
    x, g, xn = _norm_rows(ops, 8, D)
    w, b = DX.make_w(3 * D, D, device=DEV), DX.make_bias(3 * D, device=DEV)
    S = DX.exact_product(xn, w)
    gen = torch.Generator().manual_seed(D)
    fir_w = (torch.randn(3 * D, 3, generator=gen) * 0.3).bfloat16().to(DEV)
    fir_b = (torch.randn(3 * D, generator=gen) * 0.1).bfloat16().to(DEV)
    mag = 1.0 - 10.0 ** (-5.0 + 4.0 * torch.rand(D, 8, generator=gen))
    ang = (torch.rand(D, 8, generator=gen) * 2 - 1) * math.pi
    poles = torch.stack([mag * torch.cos(ang), mag * torch.sin(ang)], -1).float().contiguous().to(DEV)
    res = (torch.randn(D, 8, 2, generator=gen) * 0.25).float().contiguous().to(DEV)
    dskip = (torch.randn(D, generator=gen) * 0.5).bfloat16().to(DEV)
    worst = -1.0
    for M in (range(1, 9) if D == 4096 else Ms):                                     # (every M of the staged form for z_t; the outputs at the listed M)
        want = DX.expected(xn[:M], w, b, S=S[:M])
        outs = []
        for _ in range(2):
            fs = torch.zeros(M, 3 * D, 2, dtype=torch.bfloat16, device=DEV)
            st = torch.zeros(M, D, 8, dtype=torch.complex64, device=DEV)
            with _Spans(ops) as sp:
                y = ops.hyena_decode_fused(x[:M], g, EPS, w, b, fs, st, fir_w, fir_b, poles, res, dskip, H)
            assert sp.count == {"gemv_hyena": 1}, sp.count
            outs.append((y, fs, st))
        (y, fs, st), (y2, fs2, st2) = outs
        _exact(fs[:, :, 1].contiguous(), want, f"hyena_decode_fused M={M} D={D}: z_t")
        assert not bool(fs[:, :, 0].any())                                          # the older column: the zero state moved up
        assert torch.equal(y, y2) and torch.equal(fs, fs2) and torch.equal(torch.view_as_real(st), torch.view_as_real(st2))
        if M not in Ms:
            continue
        ry, _, nat = gpu_fft_hyena(want[:, None, :], fir_w, fir_b, poles, res, dskip, H, want_scale=True)
        ry = ry[:, 0]
        bound = ry.abs() * 2 ** -8 + ry.abs().amax(0) * 2e-3 + nat * 1e-4
        exc = float(((y.double() - ry).abs() / bound.clamp_min(1e-300)).max())
        worst = max(worst, exc)
        assert torch.isfinite(y.double()).all() and exc <= 1.0, f"M={M}: output err / row 22d's bound {exc:.3f}"
    _report(f"hyena_decode_fused D={D}", t0, n0, f", outputs worst err / bound {worst:.3f}")


def test_zz_totals():
    """The module's totals (tests/PARITY.md rows 11d / 22f are filled from these lines)."""
    dt = time.time() - TOTAL["t0"] if TOTAL["t0"] else 0.0
    print(f"[dense_exact total] exact cases {TOTAL['cases']} ({TOTAL['elements']} elements), mismatching elements {TOTAL['mismatches']}; "
          f"gate cases {TOTAL['gate_cases']}, elements outside the bound {TOTAL['gate_outside']}; wall time since the first test {dt:.1f} s")
    assert TOTAL["mismatches"] == 0 and TOTAL["gate_outside"] == 0
