"""GPU (-m gpu): the DECODE side against fp64 -- what `Generator.generate`, the hipGraph replay and `DecodePool` launch for every emitted
token -- at the positions, score regimes, filter regimes and horizons the prefill kernels are held to (tests/PARITY.md rows 22c, 15a, 22d).

 1. streaming decode attention (attn_decode_stream_kernel + attn_decode_combine_kernel) with ONE POSITION PER ROW in the real cache layout
    [B + 1, cap, 2, H, 128]: every key / value past a row's position and the whole spare row are NaN;
 2. the same kernel under the score regimes of rows 12 / 13: one spike, spike staircases across splits, a whole split 150+ log2 units
    below the rest, wide scores, shifted scores, large values;
 3. the 128-row prefill kernel (attn_fwd_kernel<false>: query ranges <= 128) under those regimes (the 8-wave kernel: test_gpu_kernels.py,
    the routing parameter of the regime tests there);
 4. the single-token Hyena launches (evo_hyena_step, evo_hyena_decode_fused_small_m at 4 and 8 rows) walked token by token through
    row 9a's 20 filter regimes x 9 scale pairs;
 5. the same launches over 8,192 consecutive steps behind an 8,193-token prompt;
 6. the angles of rope_append_decode against the fp64 cosine / sine.

Every reference is fp64 torch on the same bf16 inputs (oracle/stripedhyena_ref.py op_attention on the CPU, tests/gpu_ref64.py on the GPU).
Bounds: attention -- row 12's pins (rel-L2 <= 4e-3, |err| <= 2^-8 |ref| + 2e-2); Hyena regimes -- row 9a's; horizon -- row 6's; the fused
launch's projection -- the dense layers' (test_gpu_gemv.py::test_linear_small_m: one bf16 rounding + 2e-3 of the largest value).
"""
import math
import random
import time

import pytest
import torch

from oracle import stripedhyena_ref as R
from gpu_ref64 import gpu_fft_hyena, rmsnorm64
from test_gpu_kernels import _attn, assert_close_bf16
from test_gpu_parity_r6 import P_MODS, R_LAWS, SCALES, _regime_inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LOG2E = 1.4426950408889634
_OPS = None


def _ops():
    global _OPS
    if _OPS is None:
        from evo_amd.ops import HipOps
        _OPS = HipOps()
    return _OPS


def gen(seed):
    return torch.Generator().manual_seed(seed)


def _sync():
    if DEV != "cpu":
        torch.cuda.synchronize()


# ================================================================================================ 1 / 2: decode attention
def _judge_decode(q, kv, positions, n_splits, pre):
    """q [B, 1, H, 128] bf16 (CPU), kv [B + 1, cap, 2, H, 128] bf16 on the device, already poisoned past every row's position.  Two launches
    of the per-row form (bit-identical), finite, inside row 12's pins against R.op_attention per row over keys [0, pos[b]].
    Prescaled form: the kernel gets bf16(q c), the oracle the SAME rounded queries un-scaled (as test_gpu_kernels._attn).
    -> (the two outputs, reference [B, 1, H, 128], rel-L2 of the case or of its worst row, worst |err| - bound)."""
    ops = _ops()
    B, _, H, hd = q.shape
    assert kv.shape[0] == B + 1 and len(positions) == B and max(positions) < kv.shape[1]
    pos = torch.tensor(positions, dtype=torch.int64, device=DEV)
    c = ops.attn_q_scale(hd)
    qq = (q.float() * c).bfloat16() if pre else q
    q_ref = qq.double() / c if pre else qq
    qd = qq.to(DEV)
    outs = [ops.attention_decode(qd, kv[:B, :, 0], kv[:B, :, 1], pos=pos, n_splits=n_splits, prescaled=pre) for _ in range(2)]
    _sync()
    ref = torch.cat([R.op_attention(q_ref[b:b + 1], kv[b:b + 1, :p + 1, 0].cpu(), kv[b:b + 1, :p + 1, 1].cpu(), p)
                     for b, p in enumerate(positions)], 0)
    assert torch.isfinite(ref).all() and float(ref.abs().amax(dim=(1, 2, 3)).min()) > 1e-2, "degenerate reference"
    got = outs[0].double().cpu()
    rl2 = ((got - ref).norm() / ref.norm()).item()
    # ... and per batch row: every row is a softmax problem of its own (a row at position 0 returns v[0] exactly and carries most of a case's
    # norm; 70,000 averaged keys give outputs of 4e-3, far below the absolute term of the element bound).  One bf16 output rounding is at most
    # 2^-9 = 1.95e-3 of every element, so row 12's 4e-3 leaves the fp32 sums a factor of two
    rl2 = max(rl2, ((got - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)).max().item())
    excess = ((got - ref).abs() - (ref.abs() * 2 ** -8 + 2e-2)).max().item()
    return outs, ref, rl2, excess


def _assert_decode(outs, ref, rl2, excess, what):
    assert torch.isfinite(outs[0].float()).all(), what
    assert torch.equal(outs[0], outs[1]), f"{what}: two launches differ"
    assert rl2 <= 4e-3 and excess <= 0.0, f"{what}: rel-L2 {rl2:.3e}, |err| - (2^-8 |ref| + 2e-2) = {excess:.3e}"
    assert_close_bf16(outs[0], ref, rl2=4e-3, atol=2e-2)


def _cache(B, cap, H, positions, seed, k=None, v=None):
    """The decode cache as sh/model.py allocates it: [B + 1, cap, 2, H, 128], NaN past every row's position and in the spare row."""
    if k is None:
        g = torch.Generator(device=DEV).manual_seed(seed)
        kv = torch.randn(B + 1, cap, 2, H, 128, generator=g, device=DEV).bfloat16()
    else:
        kv = torch.stack([k, v], 2).to(DEV)
        kv = torch.cat([kv, torch.empty_like(kv[:1])], 0)
    kv[B] = float("nan")
    for b, p in enumerate(positions):
        kv[b, p + 1:] = float("nan")
    return kv


def _ragged_cases():
    """(B, cap, positions, n_splits): the edges by hand, then seeded random shapes."""
    cases = [
        (1, 1, [0], None),
        (2, 2, [1, 0], 4),
        (2, 129, [0, 128], 4),
        (3, 65, [64, 0, 33], 64),                                      # 64 splits, 2 blocks
        (3, 257, [31, 64, 256], 8),
        (1, 128, [127], 128),
        (5, 300, [0, 32, 128, 299, 65], 128),                          # more splits than key blocks
        (5, 1000, [0, 33, 65, 127, 999], None),
        (9, 2081, [0, 1, 31, 32, 33, 63, 64, 65, 2080], None),         # default: 32 splits -- the row at pos 0 leaves 31 of them empty
        (9, 3000, [127, 128, 2999, 1, 64, 700, 1500, 63, 2048], 64),
        (9, 2081, [2080, 65, 64, 63, 33, 32, 31, 1, 0], 8),
    ]
    rnd = random.Random(11)
    for _ in range(12):
        B = rnd.choice([1, 2, 3, 5, 9])
        cap = rnd.choice([2, 63, 64, 65, 127, 128, 129, 255, 257, 1000, rnd.randint(1, 3000), rnd.randint(1, 3000)])
        positions = rnd.sample(range(cap), B) if cap >= B else [rnd.randrange(cap) for _ in range(B)]
        if rnd.random() < 0.5:
            positions[rnd.randrange(B)] = cap - 1
        cases.append((B, cap, positions, rnd.choice([None, 4, 8, 64, 128])))
    return cases


_RAGGED = _ragged_cases()


@pytest.mark.parametrize("case", range(len(_RAGGED)), ids=[f"B{c[0]}-cap{c[1]}-s{c[3]}-{i}" for i, c in enumerate(_RAGGED)])
def test_decode_attention_one_position_per_row(case):
    """evo_attn_decode_bf16 as sh/model.py calls it on every pool step: one position per batch row, the full-capacity views of the real
    cache, H = 32, plain and prescaled queries.  A kernel that read dyn_pos[0] for every row fails here."""
    B, cap, positions, ns = _RAGGED[case]
    H = 32
    kv = _cache(B, cap, H, positions, 1000 + case)
    q = (torch.randn(B, 1, H, 128, generator=gen(2000 + case)) * 1.5).bfloat16()
    res = {pre: _judge_decode(q, kv, positions, ns, pre) for pre in (False, True)}
    print(f"[decode attention, per-row positions] B {B} cap {cap} pos {positions} n_splits {ns}: rel-L2 plain {res[False][2]:.3e} / prescaled "
          f"{res[True][2]:.3e}, worst |err| - bound {max(res[False][3], res[True][3]):+.2e}")
    for pre in (False, True):
        _assert_decode(*res[pre], what=f"pre={pre}")


@pytest.mark.parametrize("ns", [None, 128])
def test_decode_attention_one_position_per_row_at_full_capacity(ns):
    """cap = 131,072 (the 131k yml's cache), H = 4, positions 0 / 70,000 / 131,071 in one batch."""
    B, cap, H = 3, 131072, 4
    positions = [0, 70000, 131071]
    kv = _cache(B, cap, H, positions, 77)
    q = (torch.randn(B, 1, H, 128, generator=gen(78)) * 1.5).bfloat16()
    res = {pre: _judge_decode(q, kv, positions, ns, pre) for pre in (False, True)}
    print(f"[decode attention, per-row positions] B {B} cap {cap} pos {positions} n_splits {ns}: rel-L2 plain {res[False][2]:.3e} / prescaled "
          f"{res[True][2]:.3e}, worst |err| - bound {max(res[False][3], res[True][3]):+.2e}")
    for pre in (False, True):
        _assert_decode(*res[pre], what=f"pre={pre}")


NK2, H2 = 8192 + 37, 2
_ROW_POS = [NK2 - 1, 8192, 8223, 8224, 8200]                          # n_keys % 64 = 37, 1, 32, 33, 9
_STAIR_BLOCKS = (3, 40, 77, 110)                                       # splits 3 / 8 / 13 / 14 of 32, 3 / 0 / 5 / 6 of 8, four of 128
_SHIFT_SPLIT = 5


def _n_splits_eff(ns, cap):
    return min(((cap + 63) // 64 + 3) // 4 * 4, 32) if ns is None else ns


def _score_regime_inputs(regime, ns):
    """-> q [B, 1, H2, 128], k, v [B, NK2, H2, 128] (bf16, CPU, seeded), positions, forms.  Built on the CPU so that the fp64 reference of
    every case can be (and was) evaluated without a GPU when the seeds were chosen."""
    def base(B, seed, qs=1.0, ks=1.0, vs=1.0):
        g = gen(seed)
        return ((torch.randn(B, 1, H2, 128, generator=g) * qs).bfloat16(), (torch.randn(B, NK2, H2, 128, generator=g) * ks).bfloat16(),
                (torch.randn(B, NK2, H2, 128, generator=g) * vs).bfloat16())
    forms = (False, True)
    if regime == "spike":                                              # one key = 3 x q: key 0 | mid-block (block 45: its neighbours belong to other splits) | the last key of a ragged last half
        q, k, v = base(5, 300)
        positions = [NK2 - 1, NK2 - 1, 8192, 8223, 8224]
        for b, key in enumerate([0, 64 * 45 + 20, 8192, 8223, 8224]):
            k[b, key] = (q[b, 0].float() * 3.0).bfloat16()
    elif regime in ("staircase-ascending", "staircase-descending"):    # 1.5 / 3 / 5 / 8 x q in four different splits
        q, k, v = base(3, 310)
        positions = _ROW_POS[:3]
        muls = (1.5, 3.0, 5.0, 8.0) if regime.endswith("ascending") else (8.0, 5.0, 3.0, 1.5)
        assert len({blk % _n_splits_eff(ns, NK2) for blk in _STAIR_BLOCKS}) == 4
        for b in range(3):
            for blk, mul in zip(_STAIR_BLOCKS, muls):
                k[b, 64 * blk + 17 + b] = (q[b, 0].float() * mul).bfloat16()
    elif regime == "split-shift":                                      # every key of split 5 moved 160 log2 units down the query's direction
        q, k, v = base(3, 320, qs=2.0, ks=2.0)
        positions = _ROW_POS[:3]
        n_eff = _n_splits_eff(ns, NK2)
        c = LOG2E / math.sqrt(128.0)
        for b in range(3):
            qf = q[b, 0].float()                                       # [H2, 128]
            d = qf / (qf * qf).sum(-1, keepdim=True) * (160.0 / c)
            for blk in range(_SHIFT_SPLIT, (NK2 + 63) // 64, n_eff):
                k[b, 64 * blk:64 * blk + 64] = (k[b, 64 * blk:64 * blk + 64].float() - d).bfloat16()
    elif regime == "wide":                                             # row 13's "block 8" law
        q, k, v = base(3, 330, qs=2.5, ks=2.5)
        positions = _ROW_POS[:3]
    elif regime == "shifted":                                          # every score -81 / -19.6 / +57 log2 units from 0 (prescaled form only)
        g = gen(340)
        u = torch.randn(128, generator=g)
        u = u / u.norm() * math.sqrt(128.0)
        shifts = torch.tensor([-5.0, -1.2, 3.5])
        q = (u[None, None, None, :] + 0.05 * torch.randn(3, 1, H2, 128, generator=g)).bfloat16()
        k = (shifts[:, None, None, None] * u[None, None, None, :] + 0.3 * torch.randn(3, NK2, H2, 128, generator=g)).bfloat16()
        v = torch.randn(3, NK2, H2, 128, generator=g).bfloat16()
        positions = _ROW_POS[:3]
        forms = (True,)
    elif regime == "large-values":
        q, k, v = base(3, 350, vs=30.0)
        positions = _ROW_POS[:3]
    else:
        raise ValueError(regime)
    return q, k, v, positions, forms


SCORE_REGIMES = ["spike", "staircase-ascending", "staircase-descending", "split-shift", "wide", "shifted", "large-values"]


@pytest.mark.parametrize("ns", [None, 8, 128])
@pytest.mark.parametrize("regime", SCORE_REGIMES)
def test_decode_attention_score_regimes(regime, ns):
    """8,192 + 37 keys of capacity, H = 2, ragged positions per row: the split / combine arithmetic under the score regimes of the prefill
    kernels.  Descending staircases and the shifted split leave whole splits whose combine weight 2^(m_s - M) underflows to 0."""
    q, k, v, positions, forms = _score_regime_inputs(regime, ns)
    B = q.shape[0]
    if regime == "split-shift":                                        # the construction does what it says: the split's best key >= 150 units below the row's best
        n_eff = _n_splits_eff(ns, NK2)
        for b, p in enumerate(positions):
            s = torch.einsum("hd,khd->kh", q[b, 0].double(), k[b, :p + 1].double()) * (LOG2E / math.sqrt(128.0))
            mine = (torch.arange(p + 1) // 64) % n_eff == _SHIFT_SPLIT
            assert mine.any() and float((s[~mine].amax(0) - s[mine].amax(0)).min()) >= 150.0
    kv = _cache(B, NK2, H2, positions, 0, k, v)
    res = {pre: _judge_decode(q, kv, positions, ns, pre) for pre in forms}
    print(f"[decode attention, score regimes] {regime} n_splits {ns} pos {positions}: " + ", ".join(
        f"{'prescaled' if pre else 'plain'} rel-L2 {r[2]:.3e} worst |err| - bound {r[3]:+.2e}" for pre, r in res.items()))
    for pre in forms:
        _assert_decode(*res[pre], what=f"{regime} pre={pre}")


# ================================================================================================ 3: the 128-row prefill kernel
def _short_range_inputs(regime, Tq, Tk, seed):
    off = Tk - Tq
    g = gen(seed)
    if regime.startswith("shift"):
        shift = float(regime[5:])
        u = torch.randn(128, generator=g)
        u = u / u.norm() * math.sqrt(128.0)
        q = (u[None, None, None, :] + 0.05 * torch.randn(1, Tq, H2, 128, generator=g)).bfloat16()
        k = (shift * u[None, None, None, :] + 0.3 * torch.randn(1, Tk, H2, 128, generator=g)).bfloat16()
        v = torch.randn(1, Tk, H2, 128, generator=g).bfloat16()
        return q, k, v, (True,)
    s = 2.5 if regime == "wide" else 1.0
    q = (torch.randn(1, Tq, H2, 128, generator=g) * s).bfloat16()
    k = (torch.randn(1, Tk, H2, 128, generator=g) * s).bfloat16()
    v = torch.randn(1, Tk, H2, 128, generator=g).bfloat16()
    if regime == "spike":                                              # a key in the middle of what query row Tq // 2 sees
        row = Tq // 2
        k[0, (off + row) // 2] = (q[0, row].float() * 3.0).bfloat16()
        k[0, 0] = (q[0, Tq - 1].float() * -5.0).bfloat16()             # the last row's first key far below
    elif regime == "staircase":                                        # the last query row sees all four steps, earlier rows the first ones
        for f, mul in ((0.1, 1.5), (0.35, 3.0), (0.6, 5.0), (0.85, 8.0)):
            k[0, int(Tk * f)] = (q[0, Tq - 1].float() * mul).bfloat16()
    return q, k, v, (False, True)


@pytest.mark.parametrize("Tk", [200, 2049])
@pytest.mark.parametrize("Tq", [1, 37, 64, 128])
@pytest.mark.parametrize("regime", ["spike", "staircase", "wide", "shift-5.0", "shift-1.2", "shift3.5"])
def test_attention_short_query_ranges_under_score_regimes(regime, Tq, Tk):
    """attn_fwd_kernel<false> (query ranges <= 128: chunk continuation, short prompts, sequence-parallel shards) at q_pos0 = Tk - Tq
    under the regimes rows 12 / 13 hold the 64-rows-per-wave kernel to."""
    q, k, v, forms = _short_range_inputs(regime, Tq, Tk, 400 + Tq + Tk)
    out = []
    for pre in forms:
        o, ref = _attn(_ops(), q, k, v, Tk - Tq, pre)
        assert torch.isfinite(ref).all() and float(ref.abs().amax(-1).min()) > 1e-3
        got = o.double().cpu()
        out.append((pre, o, ref, ((got - ref).norm() / ref.norm()).item(), ((got - ref).abs() - (ref.abs() * 2 ** -8 + 2e-2)).max().item()))
    print(f"[128-row attention kernel, score regimes] {regime} Tq {Tq} Tk {Tk}: " + ", ".join(
        f"{'prescaled' if pre else 'plain'} rel-L2 {rl2:.3e} worst |err| - bound {ex:+.2e}" for pre, _, _, rl2, ex in out))
    for pre, o, ref, _, _ in out:
        assert_close_bf16(o, ref, rl2=4e-3, atol=2e-2)


# ================================================================================================ 4: single-token Hyena launches, regimes
T_REG = 2051
D_FULL = 4096


def _walk_step(z, prm, fs=None, st=None):
    """evo_hyena_step over z [B, T, 3 D], one launch per token (from zero states unless given) -> y [B, T, D], end state."""
    ops = _ops()
    fir_w, fir_b, poles, res, dskip, H = prm
    B, T, D3 = z.shape
    D = D3 // 3
    fs = torch.zeros(B, D3, 2, dtype=torch.bfloat16, device=z.device) if fs is None else fs
    st = torch.zeros(B, D, 8, dtype=torch.complex64, device=z.device) if st is None else st
    y = torch.empty(B, T, D, dtype=torch.bfloat16, device=z.device)
    for t in range(T):
        y[:, t] = ops.hyena_step(z[:, t].contiguous(), fs, st, fir_w, fir_b, poles, res, dskip, H)
    _sync()
    return y, st


def _walk_fused(xs, norm, prm, fs=None, st=None):
    """evo_hyena_decode_fused_small_m over xs [T, M, D]: the launch computes z itself, so the z_t it used is read back from fir_state
    (its newest column) after every step -> y [M, T, D], z used [M, T, 3 D], end state."""
    from evo_amd.ops import KernelTimer
    ops = _ops()
    g, eps, w, b = norm
    fir_w, fir_b, poles, res, dskip, H = prm
    T, M, D = xs.shape
    fs = torch.zeros(M, 3 * D, 2, dtype=torch.bfloat16, device=xs.device) if fs is None else fs
    st = torch.zeros(M, D, 8, dtype=torch.complex64, device=xs.device) if st is None else st
    y = torch.empty(M, T, D, dtype=torch.bfloat16, device=xs.device)
    zu = torch.empty(M, T, 3 * D, dtype=torch.bfloat16, device=xs.device)
    was = ops.timer
    ops.timer = KernelTimer()
    try:
        for t in range(T):
            y[:, t] = ops.hyena_decode_fused(xs[t], g, eps, w, b, fs, st, fir_w, fir_b, poles, res, dskip, H)
            zu[:, t] = fs[:, :, 1]
        _sync()
        assert len(ops.timer.pairs.get("gemv_hyena", ())) == T, "not the fused launch"
    finally:
        ops.timer = was
    return y, zu, st


def _projection(M, T, z_scale, seed):
    """x [T, M, D] and the pre-norm / projection parameters such that z = rmsnorm(x) W^T + b has _regime_inputs' scale `z_scale`."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    D = D_FULL
    xs = (torch.randn(T, M, D, generator=g, device=DEV) * 2).bfloat16()
    scale = (1 + 0.1 * torch.randn(D, generator=g, device=DEV)).bfloat16()
    w = (torch.randn(3 * D, D, generator=g, device=DEV) * (z_scale / math.sqrt(D))).bfloat16()
    b = (torch.randn(3 * D, generator=g, device=DEV) * 0.1 * z_scale).bfloat16()
    return xs, (scale, 1e-6, w, b)


def _judge_projection(xs, norm, zu):
    """The z rows the fused launch used vs fp64 rmsnorm64 -> projection of the step's x: one bf16 rounding + 2e-3 of the largest value.
    -> worst |err| - bound in units of the largest value."""
    g, eps, w, b = norm
    T, M, D = xs.shape
    worst = -1.0
    wd = w.double().t().contiguous()
    zmax = None
    for pass_ in (0, 1):                                               # (two passes over row chunks: the largest value first)
        m = 0.0
        for t0 in range(0, T, 1024):
            zr = rmsnorm64(xs[t0:t0 + 1024].double().reshape(-1, D), g, eps) @ wd + b.double()
            if pass_ == 0:
                m = max(m, float(zr.abs().max()))
            else:
                got = zu[:, t0:t0 + 1024].transpose(0, 1).reshape(-1, 3 * D).double()
                worst = max(worst, float((((got - zr).abs() - (zr.abs() * 2 ** -8 + 2e-3 * zmax)) / zmax).max()))
        zmax = m if pass_ == 0 else zmax
    return worst


def _judge_regimes(y, st, ry, rst, nat, rfloor, reg, worst, bad, tag):
    """Row 9a's per-regime judgement (tests/test_gpu_parity_r6.py), every channel: outputs inside |ref| 2^-8 + 2e-3 cmax + 1e-4 nat,
    rel-L2 <= 2.2e-3 and <= 1.05 x the eager-bf16 floor, end state within 1e-4 of the channel's largest component."""
    nreg = len(P_MODS) * len(R_LAWS)
    yd = y.double()
    assert torch.isfinite(yd).all(), tag
    cmax = ry.abs().amax(dim=(0, 1))
    bound = ry.abs() * 2 ** -8 + cmax * 2e-3 + nat * 1e-4
    smax = rst.abs().amax(dim=(0, 2))
    exc = (((yd - ry).abs() - bound) / cmax.clamp_min(1e-300)).amax(dim=(0, 1))
    serr = (st.to(torch.complex128) - rst).abs().amax(dim=(0, 2)) / smax.clamp_min(1e-300)
    for k in range(nreg):
        sel = reg == k
        key = (P_MODS[k % len(P_MODS)], R_LAWS[k // len(P_MODS)])
        rl2 = ((yd[..., sel] - ry[..., sel]).norm() / ry[..., sel].norm()).item()
        fl2 = ((rfloor[..., sel] - ry[..., sel]).norm() / ry[..., sel].norm()).item()
        ex, se = exc[sel].max().item(), serr[sel].max().item()
        w = worst.get(key, (0.0, 0.0, -1.0, 0.0))
        worst[key] = (max(w[0], rl2), max(w[1], rl2 / fl2), max(w[2], ex), max(w[3], se))
        if not (ex <= 0.0 and rl2 <= 2.2e-3 and rl2 <= 1.05 * fl2 and se <= 1e-4):
            bad.append(dict(tag=tag, p_mod=key[0], residues=key[1], rel_l2=rl2, floor=fl2, excess=ex, state=se))


def _print_regimes(name, worst, dt, extra=""):
    print(f"[hyena single-token regimes, {name}] 20 regimes x 9 scale pairs, {T_REG} launches each, in {dt:.0f} s{extra}; per regime (worst over "
          f"the scale pairs): y rel-L2 | rel-L2 / eager-bf16 floor | excess over the bf16 bound | end-state err / channel max")
    for law in R_LAWS:
        print(f"[hyena single-token regimes, {name}] residues {law:6s}: " + "  ".join(
            f"|p|={pm:g}: {worst[(pm, law)][0]:.2e} {worst[(pm, law)][1]:.2f} {worst[(pm, law)][2]:+.1e} {worst[(pm, law)][3]:.1e}" for pm in P_MODS))


def test_hyena_step_walks_the_parameter_regimes_vs_fft():
    """evo_hyena_step, M = 2, D = 4096: T_REG tokens one launch at a time from zero states, every y_t and the final modal state against the
    fp64 FFT long convolution over the whole sequence -- row 9a's regimes, inputs and judgement.  fp32 modal states, no operand-table guard:
    every regime must hold, no channel is left out."""
    worst, bad = {}, []
    t0 = time.time()
    for zi, zs in enumerate(SCALES):
        for fi, fs_ in enumerate(SCALES):
            z, prm, reg = _regime_inputs(2, T_REG, zs, fs_, 100 + 10 * zi + fi)
            ry, rst, nat = gpu_fft_hyena(z, *prm, want_scale=True)
            rfloor, _ = gpu_fft_hyena(z, *prm, ref_rounding=True, want_state=False)
            assert torch.isfinite(ry).all() and torch.isfinite(rst.real).all()
            y, st = _walk_step(z, prm)
            _judge_regimes(y, st, ry, rst, nat, rfloor, reg, worst, bad, f"z x {zs:g}, fir x {fs_:g}")
            del ry, rst, rfloor, z, y
    _print_regimes("hyena_step M=2", worst, time.time() - t0)
    for b_ in bad[:12]:
        print("[hyena single-token regimes] OUTSIDE THE BOUND:", b_)
    assert not bad, bad[:6]


@pytest.mark.parametrize("M", [4, 8])
def test_hyena_decode_fused_walks_the_parameter_regimes_vs_fft(M):
    """evo_hyena_decode_fused_small_m at D = 4096 with 4 and 8 rows (8: the LDS-staged form): the z_t of every step (read back from
    fir_state) against the fp64 norm -> projection of the step's x, y_t and the final state against the fp64 recurrence on exactly those z
    rows -- row 9a's regimes and judgement."""
    worst, bad = {}, []
    zworst = -1.0
    t0 = time.time()
    for zi, zs in enumerate(SCALES):
        for fi, fs_ in enumerate(SCALES):
            _, prm, reg = _regime_inputs(1, 1, zs, fs_, 100 + 10 * zi + fi)
            xs, norm = _projection(M, T_REG, zs, 500 + 10 * zi + fi)
            y, zu, st = _walk_fused(xs, norm, prm)
            zw = _judge_projection(xs, norm, zu)
            zworst = max(zworst, zw)
            assert zw <= 0.0, (zs, fs_, zw)
            ry, rst, nat = gpu_fft_hyena(zu, *prm, want_scale=True)
            rfloor, _ = gpu_fft_hyena(zu, *prm, ref_rounding=True, want_state=False)
            assert torch.isfinite(ry).all() and torch.isfinite(rst.real).all()
            _judge_regimes(y, st, ry, rst, nat, rfloor, reg, worst, bad, f"z x {zs:g}, fir x {fs_:g}")
            del ry, rst, rfloor, y, zu, xs
    _print_regimes(f"hyena_decode_fused M={M}", worst, time.time() - t0,
                   f"; z_t vs fp64 norm -> projection: worst |err| - (2^-8 |ref| + 2e-3 max) = {zworst:+.1e} max")
    for b_ in bad[:12]:
        print("[hyena single-token regimes] OUTSIDE THE BOUND:", b_)
    assert not bad, bad[:6]


# ================================================================================================ 5: long horizons
T_PROMPT, N_DEC = 8193, 8192


def _horizon_params(seed, one_minus=None):
    """The default synthetic law at D = 4096 (test_gpu_fulldepth._hyena_inputs: |p| = 1 - 10^U(-5,-1), residues ~ sqrt(1 - |p|)); or every
    channel at |p| = 1 - one_minus."""
    g = torch.Generator(device=DEV).manual_seed(seed)
    D, H = D_FULL, 32
    fir_w = (torch.randn(3 * D, 3, generator=g, device=DEV) * 0.3).bfloat16()
    fir_b = (torch.randn(3 * D, generator=g, device=DEV) * 0.1).bfloat16()
    om = 10.0 ** (-5.0 + 4.0 * torch.rand(D, 8, generator=g, device=DEV))
    if one_minus is not None:
        om = torch.full_like(om, one_minus)
    mag = 1.0 - om
    ang = (torch.rand(D, 8, generator=g, device=DEV) * 2 - 1) * math.pi
    poles = torch.stack([mag * torch.cos(ang), mag * torch.sin(ang)], -1).float().contiguous()
    res = (torch.randn(D, 8, 2, generator=g, device=DEV) * torch.sqrt(om).unsqueeze(-1)).float().contiguous()
    dskip = (torch.randn(D, generator=g, device=DEV) * 0.5).bfloat16()
    return fir_w, fir_b, poles, res, dskip, H


def _fp32_torch_recurrence_state(z, prm):
    """The reference's recurrent arithmetic, plain fp32 torch on the GPU: s <- p s + x1 v over every token of z [1, T, 3 D] from zero
    (x1 v from the fp64 FIR, rounded once to fp32).  -> end state [1, D, 8] complex64."""
    fir_w, fir_b, poles, _, _, H = prm
    B, T, D3 = z.shape
    D = D3 // 3
    zz = torch.nn.functional.pad(z.double(), (0, 0, 2, 0))
    w = fir_w.double()
    f = (w[:, 0] * zz[:, 0:T] + w[:, 1] * zz[:, 1:T + 1] + w[:, 2] * zz[:, 2:T + 2] + fir_b.double()).view(B, T, H, 3, D // H)
    x1v = (f[:, :, :, 1] * f[:, :, :, 2]).reshape(B, T, D).float()
    del zz, f
    p = torch.view_as_complex(poles.contiguous())
    s = torch.zeros(B, D, 8, dtype=torch.complex64, device=z.device)
    for t in range(T):
        s = p * s + x1v[:, t, :, None]
    return s


@pytest.mark.parametrize("law", ["default", "all-1-1e-6"])
@pytest.mark.parametrize("path", ["hyena_step-M1", "hyena_decode_fused-M8"])
def test_single_token_hyena_launches_over_an_8192_step_horizon(path, law):
    """A generation of thousands of nucleotides is the single-token launch applied thousands of times to its own fp32 state: an 8,193-token
    prompt through hyena_ct (tail form) seeds the modal state and the FIR history, then 8,192 consecutive launches.  Against the fp64 FFT
    long convolution over all 16,385 tokens (tests/gpu_ref64.py, channel chunks): row 6's pins on the decode outputs and the final state,
    and the error of the last 1,024 steps no more than 1.1 x that of the first 1,024."""
    from evo_amd.hyena_tables import mfma_operand_table
    ops = _ops()
    M = 1 if path.endswith("M1") else 8
    D, T, N = D_FULL, T_PROMPT, N_DEC
    prm = _horizon_params(31 if law == "default" else 32, None if law == "default" else 1e-6)
    fir_w, fir_b, poles, res, dskip, H = prm
    g = torch.Generator(device=DEV).manual_seed(33 + M)
    zp = torch.randn(M, T, 3 * D, generator=g, device=DEV).bfloat16()
    t0 = time.time()
    zt = ops.zt_from_rows(zp, M, T, float("nan"))
    assert ops.zt_layout(M, T)[3] == 1                                 # tail form
    _, st = ops.hyena_ct(zt, M, T, fir_w, fir_b, mfma_operand_table(poles, res, dskip), H, want_state=True, poles=poles)
    del zt
    st = st.contiguous()
    fs = zp[:, T - 2:T].transpose(1, 2).contiguous()                   # [M, 3 D, 2], oldest first
    zmsg = ""
    if M == 1:
        zd = torch.randn(M, N, 3 * D, generator=g, device=DEV).bfloat16()
        y, st = _walk_step(zd, prm, fs, st)
    else:
        xs, norm = _projection(M, N, 1.0, 40)
        y, zd, st = _walk_fused(xs, norm, prm, fs, st)
        zw = _judge_projection(xs, norm, zd)
        zmsg = f"; z_t vs fp64 norm -> projection: worst |err| - bound {zw:+.1e} max"
        assert zw <= 0.0, zw
        del xs
    t_run = time.time() - t0
    z_all = torch.cat([zp, zd], 1)
    del zp, zd
    ry, rst = gpu_fft_hyena(z_all, *prm)
    ry = ry[:, T:]
    yd = y.double()
    assert torch.isfinite(yd).all()
    err = (yd - ry).abs()
    rl2 = (err.norm() / ry.norm()).item()
    excess = (err - (ry.abs() * 2 ** -8 + float(ry.abs().max()) * 2e-3)).max().item()
    first = ((yd[:, :1024] - ry[:, :1024]).norm() / ry[:, :1024].norm()).item()
    last = ((yd[:, -1024:] - ry[:, -1024:]).norm() / ry[:, -1024:].norm()).item()
    srel = ((st.to(torch.complex128) - rst).abs().max() / rst.abs().max()).item()
    msg = (f"[hyena single-token horizon, {path}, poles {law}] {T}-token prompt + {N} launches ({t_run:.1f} s, reference {time.time() - t0 - t_run:.1f} s): "
           f"y rel-L2 {rl2:.3e} (first / last 1,024 steps {first:.3e} / {last:.3e}), worst excess over the bf16 bound {excess:.3e}, "
           f"end-state rel {srel:.2e}{zmsg}")
    if M == 1:                                                         # the same recurrence in plain fp32 torch: what the reference's arithmetic holds
        s32 = _fp32_torch_recurrence_state(z_all, prm)
        msg += f"; plain fp32 torch recurrence over the {T + N} tokens: end-state rel {((s32.to(torch.complex128) - rst).abs().max() / rst.abs().max()).item():.2e}"
    print(msg)
    assert rl2 <= 2e-3 and excess <= 0.0, (rl2, excess)
    assert last <= 1.1 * first, (first, last)
    assert srel <= 2e-5, srel


# ================================================================================================ 6: rotary angles
def _bf16_neighbourhood(v):
    """v fp64 -> (e: v rounded to bf16, ulp: the bf16 spacing at e, dist: |v| to the rounding boundary between e and its neighbour on
    v's side)."""
    e = v.float().bfloat16().double()
    a = e.abs()
    m, ex = torch.frexp(a)
    ulp = torch.ldexp(torch.ones_like(a), ex - 8)
    down = torch.where(m > 0.5, ulp / 2, ulp / 4)                      # (below a power of two the spacing halves)
    mid = torch.where(v.abs() >= a, a + ulp / 2, a - down)
    return e, ulp, (v.abs() - mid).abs()


@pytest.mark.parametrize("scaling", [1.0, 16.0])
def test_rope_append_decode_angles_vs_fp64_cosine(scaling):
    """q and k rows (1 .. 1, 0 .. 0), q_scale = 1: the stored k row is exactly (bf16(cos f), bf16(sin f)).  Against bf16 of the fp64 cosine /
    sine of the fp32 angle the kernel forms (float(p) / scaling * inv_freq): an entry may differ by one bf16 ulp, and only where the fp64
    value lies within 2^-21 of a rounding boundary -- room for a few fp32 ulps of cosf / sinf at angles up to 1.3e5 rad, three orders of
    magnitude below a bf16 step.  (torch's fp32 cos / sin on the CPU meet the same condition at these positions with no differing entry.)
    test_rope_append_decode_is_bitwise_table_rope_and_indexed_copy carries the result over to the table path."""
    ops = _ops()
    positions = [0, 1, 8191, 60000, 70000, 131071]
    B, H, hd = len(positions), 2, 128
    qkv = torch.zeros(B, 1, 3, H, hd, dtype=torch.bfloat16, device=DEV)
    qkv[:, :, :2, :, :hd // 2] = 1.0
    kv = torch.zeros(B + 1, max(positions) + 1, 2, H, hd, dtype=torch.bfloat16, device=DEV)
    pos = torch.tensor(positions, dtype=torch.int64, device=DEV)
    inv = (1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))).to(DEV)
    ops.rope_append_decode(qkv, kv[:B], pos, inv, scaling, q_scale=1.0)
    _sync()
    krow = kv[torch.arange(B, device=DEV), pos, 0].cpu()               # [B, H, hd]
    assert torch.equal(qkv[:, 0, 0].cpu(), krow) and torch.equal(qkv[:, 0, 1].cpu(), krow)
    t = torch.tensor(positions, dtype=torch.float32)
    if scaling != 1.0:
        t = t / scaling
    f = (t[:, None] * inv.cpu()[None, :]).double()                     # the fp32 angle, exactly
    n_diff, closest = 0, float("inf")
    for name, v, got in (("cos", torch.cos(f), krow[..., :hd // 2]), ("sin", torch.sin(f), krow[..., hd // 2:])):
        e, ulp, dist = _bf16_neighbourhood(v)
        for h in range(H):
            gd = got[:, h].double()
            diff = gd != e
            n_diff += int(diff.sum())
            assert ((gd - e).abs() <= ulp).all(), name
            assert (dist[diff] <= 2.0 ** -21).all(), (name, h, dist[diff].max().item())
        closest = min(closest, float(dist.min()))
    print(f"[rope_append_decode angles, scaling {scaling:g}] positions {positions}: {n_diff} of {2 * B * H * (hd // 2)} entries differ from bf16 of the "
          f"fp64 cosine / sine (each within 2^-21 of a rounding boundary; the closest any value comes to one: {closest:.1e})")
