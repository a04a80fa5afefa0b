"""GPU (-m gpu): the fused single-token Hyena launches on EXACT sums (tests/hyena_fused_exact.py; PARITY row 9e) -- outputs AND both carried
states after every step, against the per-step fp64 recurrence, with no tolerance term.

evo_hyena_decode_fused_small_m (bf16 weights, HipOps.hyena_decode_fused) and evo_hyena_decode_fused_small_m_w8 (FP8 weights,
HipOps.hyena_decode_fused_w8) do pre-norm -> projection + bias -> FIR step -> modal step -> gate in one launch.  The token rows are made so
that the launch's own norm and projection produce a member of family U (40 steps) or I (140 steps, impulses in the first 40) exactly
(tests/test_hyena_fused_exact_host.py), from a NON-ZERO FIR history and modal state.  After every step t:
  y_t        == round_store(ref.y[:, t]) as values (the same bit pattern, -0 == +0; NaN equals nothing)
  fir_state  == [z_(t-1) | z_t], bit for bit
  iir_state  == ref.states[:, t] cast to complex64 (exact), by hyena_exact's flush rule: family I's tiny region 0 < |ref| < 2^-100 is
                held to |got| <= 2^-99, never skipped
Every walk runs twice in lockstep on its own buffers; the two must hold the same BITS in y, fir_state and iir_state after every step.  The
state buffers carry one more row of a sentinel behind the M rows passed; it must keep its bits.  Comparisons run on the device; a walk
synchronises once, at its end.  The launch timer's spans prove the fused launch ran: one per step and run.

test_tail_is_bitwise_hyena_step: the FIR / modal / gate arithmetic of EVERY form against evo_hyena_step (exact-tested itself in
tests/test_gpu_hyena_exact.py, section e) on random data and random non-zero states, three steps, on bit views -- the check that replaces
the 2^-6 tolerance of tests/test_gpu_gemv.py / tests/test_gpu_w8.py at M = 5 .. 8 and for FP8.  D = 512: 64 vectors; D = 2176: 272 vectors
(FP8: 136), the unstaged loop with a refill and a tail slice.

Instantiation -> the test that reaches it (for_m_stage: staged M = 1 .. 8, unstaged M = 1 .. 4; twelve per entry):
  gemv_norm_hyena_kernel<1..8, 1, true>         test_walk[bf16-{U,I}-4096-1..8]            test_tail_is_bitwise_hyena_step[bf16-4096-1..8]
  gemv_norm_hyena_kernel<1, 1, false>           test_walk[bf16-{U,I}-{256,1024}-1]         test_tail_is_bitwise_hyena_step[bf16-{256,512,1024,2176}-1]
  gemv_norm_hyena_kernel<2, 2, false>           test_walk[bf16-{U,I}-{256,1024}-2]         test_tail_is_bitwise_hyena_step[bf16-{256,512,1024,2176}-2]
  gemv_norm_hyena_kernel<3, 2, false>           test_walk[bf16-{U,I}-{256,1024}-3]         test_tail_is_bitwise_hyena_step[bf16-{256,512,1024,2176}-3]
  gemv_norm_hyena_kernel<4, 1, false>           test_walk[bf16-{U,I}-{256,1024}-4]         test_tail_is_bitwise_hyena_step[bf16-{256,512,1024,2176}-4]
  w8_gemv_norm_hyena_kernel<1..8, 1, true>      test_walk[w8-{U,I}-4096-1..8]              test_tail_is_bitwise_hyena_step[w8-4096-1..8]
  w8_gemv_norm_hyena_kernel<1, 1, false>        test_walk[w8-{U,I}-{256,1024}-1]           test_tail_is_bitwise_hyena_step[w8-{256,512,1024,2176}-1]
  w8_gemv_norm_hyena_kernel<2, 2, false>        test_walk[w8-{U,I}-{256,1024}-2]           test_tail_is_bitwise_hyena_step[w8-{256,512,1024,2176}-2]
  w8_gemv_norm_hyena_kernel<3, 2, false>        test_walk[w8-{U,I}-{256,1024}-3]           test_tail_is_bitwise_hyena_step[w8-{256,512,1024,2176}-3]
  w8_gemv_norm_hyena_kernel<4, 1, false>        test_walk[w8-{U,I}-{256,1024}-4]           test_tail_is_bitwise_hyena_step[w8-{256,512,1024,2176}-4]
"""
import math
import time

import pytest
import torch

import dense_exact as DX
import hyena_exact as X
import hyena_fused_exact as F
from evo_amd.sh.cache import fp8_row_rule

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
EPS = DX.EPS
SENT = 7.0
SPAN = {"bf16": "gemv_hyena", "w8": "gemv_hyena_w8"}
TOTAL = {"t0": None, "launches": 0, "elements": 0, "tiny": 0, "mismatches": 0}
CELLS = [pytest.param(D, M, id=f"{D}-{M}") for D, Ms in F.SHAPES for M in Ms]
TAIL_CELLS = [pytest.param(D, M, id=f"{D}-{M}") for D, Ms in [(4096, range(1, 9))] + [(D, range(1, 5)) for D in (256, 512, 1024, 2176)] for M in Ms]


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


def _bits(t):
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


class Case:
    """One (family, D) data set on the device, built once: the token rows, W and its FP8 record, the filters, the start states and what
    every step must leave (y rounded once to bf16, the history as bf16, the modal states as complex64 -- all exact casts)."""
    _cache = {}

    def __init__(self, ops, fam, D):
        c = F.make(fam, D)                                                # on the CPU: the family's conditions are asserted on the way
        d = lambda t: t.to(DEV)
        self.fam, self.D, self.H, self.T = fam, D, c.H, c.z.shape[1]
        self.xs, self.g, self.W, self.b = d(c.xs), d(c.g), d(c.W), d(c.b)
        self.prm = tuple(d(t) for t in c.prm)
        self.fs0 = d(c.hist.transpose(1, 2).contiguous())                 # [M, 3 D, 2]
        self.st0 = d(c.s0.to(torch.complex64))
        self.want_y = d(X.round_store(c.ref.y))                           # [M, T, D] bf16
        self.hist = d(c.ref.hist.to(BF))                                  # [M, T + 2, 3 D]
        self.want_st = d(torch.view_as_real(c.ref.states.to(torch.complex64)).contiguous())      # [M, T, D, 8, 2] f32
        self.rec = ops.w_quant_fp8(self.W)
        data, scale = fp8_row_rule(c.W)
        assert torch.equal(self.rec.data.cpu(), data) and torch.equal(self.rec.scale.cpu(), scale)
        assert torch.equal(_bits(self.rec.dequantize()), _bits(self.W)), "W is not a fixed point of the FP8 rule"

    @classmethod
    def get(cls, ops, fam, D):
        if (fam, D) not in cls._cache:
            cls._cache[fam, D] = cls(ops, fam, D)
        return cls._cache[fam, D]


def _step_fn(ops, entry, c):
    if entry == "bf16":
        return lambda x, fs, st: ops.hyena_decode_fused(x, c.g, EPS, c.W, c.b, fs, st, *c.prm, c.H)
    return lambda x, fs, st: ops.hyena_decode_fused_w8(x, c.g, EPS, c.rec, c.b, fs, st, *c.prm, c.H)


def _ok(fam, got, ref):
    """(elementwise ok, elements under the flush rule [0-dim tensor]) -- no host synchronisation."""
    if fam == "U":
        return got == ref, torch.zeros((), dtype=torch.int64, device=got.device)
    ok, tiny = X.flushed_ok(got, ref)
    return ok, tiny.sum()


# ================================================================================================ the exact walks
@pytest.mark.parametrize("D,M", CELLS)
@pytest.mark.parametrize("fam", ["U", "I"])
@pytest.mark.parametrize("entry", ["bf16", "w8"])
def test_walk(entry, fam, D, M):
    ops = _ops()
    c = Case.get(ops, fam, D)
    step, T = _step_fn(ops, entry, c), c.T
    runs = []
    for _ in range(2):
        fs = torch.full((M + 1, 3 * D, 2), SENT, dtype=BF, device=DEV)
        st = torch.full((M + 1, D, 8), complex(SENT, -SENT), dtype=torch.complex64, device=DEV)
        fs[:M], st[:M] = c.fs0[:M], c.st0[:M]
        runs.append((fs, st))
    bad = torch.zeros(T, 4, dtype=torch.int64, device=DEV)               # per step: y, fir_state, iir_state, run 1 against run 2
    n_tiny = torch.zeros((), dtype=torch.int64, device=DEV)
    with _Spans(ops) as sp:
        for t in range(T):
            x = c.xs[t, :M]
            (ya, yb) = [step(x, fs[:M], st[:M]) for fs, st in runs]
            (fa, sa), (fb, sb) = runs
            ok_y, ty = _ok(fam, ya, c.want_y[:M, t])
            want_fir = torch.stack([c.hist[:M, t + 1], c.hist[:M, t + 2]], -1)
            ok_s, ts = _ok(fam, torch.view_as_real(sa[:M]), c.want_st[:M, t])
            bad[t, 0] = (~ok_y).sum()
            bad[t, 1] = (_bits(fa[:M]) != _bits(want_fir)).sum()
            bad[t, 2] = (~ok_s).sum()
            bad[t, 3] = (_bits(ya) != _bits(yb)).sum() + (_bits(fa) != _bits(fb)).sum() + (_bits(sa) != _bits(sb)).sum()
            n_tiny += ty + ts
    assert sp.count == {SPAN[entry]: 2 * T}, sp.count                     # the fused launch ran, once per step and run
    bad = bad.cpu()                                                       # (the walk's one synchronisation)
    per_step = M * D + M * 3 * D * 2 + M * D * 16
    TOTAL["launches"] += 2 * T
    TOTAL["elements"] += T * per_step
    TOTAL["tiny"] += int(n_tiny)
    TOTAL["mismatches"] += int(bad[:, :3].sum())
    for fs, st in runs:
        assert bool((fs[M] == SENT).all()) and bool((torch.view_as_real(st[M]) == torch.tensor([SENT, -SENT], device=DEV)).all()), \
            "the row behind the M rows passed was written"
    if int(bad.sum()):
        t = int(bad.sum(1).nonzero()[0])
        names = ("y", "fir_state", "iir_state", "run 1 against run 2")
        first = ", ".join(f"{n}: {int(v)}" for n, v in zip(names, bad[t]) if int(v))
        tot = ", ".join(f"{n}: {int(v)} elements in {int((bad[:, i] != 0).sum())} steps" for i, (n, v) in enumerate(zip(names, bad.sum(0))) if int(v))
        pytest.fail(f"{entry} {fam} D={D} M={M}: first differing step {t} ({first} of {per_step} elements); over {T} steps {tot}", pytrace=False)


# ================================================================================================ the tail against evo_hyena_step, every form
_RANDOM = {}


def _random(ops, D):
    """Random weights, filters and states as in tests/test_gpu_gemv.py, once per D (8 rows; a test takes its first M)."""
    if D not in _RANDOM:
        g = torch.Generator().manual_seed(1000 + D)
        d = lambda t: t.to(DEV)
        scale = d((1 + 0.1 * torch.randn(D, generator=g)).bfloat16())
        w = d((torch.randn(3 * D, D, generator=g) / D ** 0.5).bfloat16())
        b = d((torch.randn(3 * D, generator=g) * 0.1).bfloat16())
        fir_w = d((torch.randn(3 * D, 3, generator=g) * 0.3).bfloat16())
        fir_b = d((torch.randn(3 * D, generator=g) * 0.1).bfloat16())
        mag = 1.0 - 10.0 ** (-5.0 + 4.0 * torch.rand(D, 8, generator=g))
        ang = (torch.rand(D, 8, generator=g) * 2 - 1) * math.pi
        poles = d(torch.stack([mag * torch.cos(ang), mag * torch.sin(ang)], -1).float().contiguous())
        res = d((torch.randn(D, 8, 2, generator=g) * 0.25).float().contiguous())
        dskip = d((torch.randn(D, generator=g) * 0.5).bfloat16())
        fs = d(torch.randn(8, 3 * D, 2, generator=g).bfloat16())
        st = d(torch.view_as_complex(torch.randn(8, D, 8, 2, generator=g).contiguous()))
        xs = d((torch.randn(3, 8, D, generator=g) * 2).bfloat16())
        assert D % 16 == 0                                                # (what w_quant_fp8 asks of K; 2176 = 136 * 16)
        _RANDOM[D] = dict(scale=scale, w=w, rec=ops.w_quant_fp8(w), b=b, prm=(fir_w, fir_b, poles, res, dskip), fs=fs, st=st, xs=xs)
    return _RANDOM[D]


@pytest.mark.parametrize("D,M", TAIL_CELLS)
@pytest.mark.parametrize("entry", ["bf16", "w8"])
def test_tail_is_bitwise_hyena_step(entry, D, M):
    """Per step: clone the states, run the fused launch, read the z_t it computed back from fir_state's newest column, run evo_hyena_step
    on that z_t from the cloned states: y, fir_state and iir_state are the same bits."""
    ops = _ops()
    r, H = _random(ops, D), D // 128
    fs, st = r["fs"][:M].clone(), r["st"][:M].clone()
    assert bool(fs.any()) and bool(torch.view_as_real(st).all())
    with _Spans(ops) as sp:
        for t in range(3):
            x = r["xs"][t, :M]
            fs2, st2 = fs.clone(), st.clone()
            if entry == "bf16":
                y = ops.hyena_decode_fused(x, r["scale"], 1e-6, r["w"], r["b"], fs, st, *r["prm"], H)
            else:
                y = ops.hyena_decode_fused_w8(x, r["scale"], 1e-6, r["rec"], r["b"], fs, st, *r["prm"], H)
            z_t = fs[:, :, 1].contiguous()
            y2 = ops.hyena_step(z_t, fs2, st2, *r["prm"], H)
            assert torch.equal(_bits(y), _bits(y2)), f"step {t}: y, {int((_bits(y) != _bits(y2)).sum())} of {y.numel()} differ"
            assert torch.equal(_bits(fs), _bits(fs2)), f"step {t}: fir_state"
            assert torch.equal(_bits(st), _bits(st2)), f"step {t}: iir_state, {int((_bits(st) != _bits(st2)).sum())} of {2 * st.numel()} differ"
            assert bool(torch.isfinite(y.float()).all())
    assert sp.count.get(SPAN[entry]) == 3, sp.count
    TOTAL["launches"] += 3


def test_zz_totals():
    """The module's totals (tests/PARITY.md row 9e is filled from this line)."""
    dt = time.time() - TOTAL["t0"] if TOTAL["t0"] else 0.0
    print(f"[hyena_fused_exact total] launches {TOTAL['launches']}, elements compared {TOTAL['elements']}, of them in family I's tiny region "
          f"{TOTAL['tiny']}, mismatching elements {TOTAL['mismatches']}; wall time since the first test {dt:.1f} s")
