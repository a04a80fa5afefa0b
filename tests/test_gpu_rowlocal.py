"""Row-local kernels against fp64, element by element (PARITY.md rows 24a-24d): the fused scoring tail and evo_logprob_entropy on
logits that are EXACT (any summation order, bf16), the GELU gate on every finite bf16 input, RMSNorm / rms_finalize / rmsnorm_rows at
widths where the `idx < nvec` guards turn false inside a wave and past the 16,384-block grid cap, and the rotary kernel with two
passes of its `j` loop and past its 65,536-block cap.  Inputs, references and bounds: tests/rowlocal_ref.py (pinned on the CPU by
tests/test_rowlocal_host.py).  No bound here has a tensor-wide `max` term.

MI355X, the `[rowlocal ...]` lines of this module: PARITY.md rows 24a-24d.
"""
import math

import pytest
import torch

import rowlocal_ref as RL

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def ops():
    from evo_amd.ops import HipOps
    return HipOps()


# =========================================================================================== 1. scoring tail on exact logits
SEL_SETS = {1: (RL.ANTI_T,), 3: (0, RL.ANTI_C, 391), 8: RL.TIE_COLS + (RL.ANTI_T, RL.ANTI_C, 5, 511)}


def _worst(got, ref, allow):
    """(largest |got - ref|, largest |got - ref| / allowance) of an fp32 kernel output against its fp64 reference."""
    err = (got.double() - ref).abs()
    assert bool(torch.isfinite(got).all())
    return float(err.max()), float((err / allow).max())


@pytest.mark.parametrize("K", [32, 288, 4096])
@pytest.mark.parametrize("M", [1, 63, 64, 65, 1061])
def test_scoring_tail_on_exact_logits_vs_fp64_per_row(ops, M, K):
    """evo_unembed_logprob_bf16, evo_unembed_profile_bf16 (n_sel 1 / 3 / 8, the planted columns among the ids) and
    evo_linear -> evo_logprob_entropy (bf16 and f32 logits) on rowlocal_ref.exact_logit_case: every logit is a multiple of 1/8 inside
    +-32, so the kernels' rounded logits ARE the fp64 logits and log-prob, entropy and every selected column are judged per row
    against fp64 log_softmax.  Allowance (measured in the same run, rowlocal_ref.measured_allowance): 4 x the largest error of the same
    formula in eager fp32 torch on the same logits, floor 2^-22 (1 + |ref|).  The three entry points see identical logits and must agree
    with each other inside the same allowance.  Planted rows: one dominant column in every wave and lane half (target on it), a flat
    row, the maximum tied across the four waves, the target on a -32 column under a +32 one."""
    c = RL.exact_logit_case(M, K)
    if M == 1061:                                                           # HOST, before any launch: every column is a target in both halves
        assert int(RL.target_coverage(c["target"]).min()) >= 1
    hid, emb, tgt = c["hidden"].to(DEV), c["emb"].to(DEV), c["target"].to(DEV)
    lg = RL.logits64(hid, emb)
    assert torch.equal(lg.to(torch.bfloat16).double(), lg) and float(lg.abs().max()) <= 32
    ref_lp, ref_en, _ = RL.logprob_entropy64(lg, tgt)
    f_lp, f_en, _ = RL.logprob_entropy_f32(lg, tgt)
    a_lp, e32_lp = RL.measured_allowance(ref_lp, f_lp)
    a_en, e32_en = RL.measured_allowance(ref_en, f_en)
    worst = {}

    def judge(name, lp, en):
        worst[name] = (_worst(lp, ref_lp, a_lp), _worst(en, ref_en, a_en))

    lp0, en0 = ops.unembed_logprob(hid, emb, tgt, want_logprob=True, want_entropy=True)
    judge("tail", lp0, en0)
    sel_worst = (0.0, 0.0)
    for n_sel, ids in SEL_SETS.items():
        _, _, ref_sl = RL.logprob_entropy64(lg, None, sel=ids)
        _, _, f_sl = RL.logprob_entropy_f32(lg, None, sel=ids)
        a_sl, _ = RL.measured_allowance(ref_sl, f_sl)
        sl, lp, en = ops.unembed_profile(hid, emb, ids, tgt)
        assert sl.shape == (M, n_sel)
        judge(f"profile{n_sel}", lp, en)
        sel_worst = max(sel_worst, _worst(sl, ref_sl, a_sl), key=lambda t: t[1])
        assert torch.equal(lp, lp0) and torch.equal(en, en0)               # (the profile launch's row statistics are the tail's, bit for bit)
    logits = ops.linear(hid, emb, None)
    assert torch.equal(logits.double(), lg)                                 # the dense layer's logits are exact too: same inputs for both paths
    lp_b, en_b = ops.logprob_entropy(logits, tgt, want_logprob=True, want_entropy=True)
    judge("two-kernel bf16", lp_b, en_b)
    lp_f, en_f = ops.logprob_entropy(logits.float(), tgt, want_logprob=True, want_entropy=True)
    judge("two-kernel f32", lp_f, en_f)
    agree = max(float(((lp0 - x).abs().double() / a_lp).max()) for x in (lp_b, lp_f))
    agree = max(agree, max(float(((en0 - x).abs().double() / a_en).max()) for x in (en_b, en_f)))
    w_lp = max(v[0] for v in worst.values())
    w_en = max(v[1] for v in worst.values())
    print(f"[rowlocal scoring M={M} K={K}] fp32 restatement err: log-prob {e32_lp:.2e}, entropy {e32_en:.2e}; kernels worst err "
          f"log-prob {w_lp[0]:.2e} ({w_lp[1]:.2f} of the allowance), entropy {w_en[0]:.2e} ({w_en[1]:.2f}), selected columns "
          f"{sel_worst[0]:.2e} ({sel_worst[1]:.2f}); entry points agree to {agree:.2f} of the allowance")
    for name, (wl, we) in worst.items():
        assert wl[1] <= 1.0, (name, "log-prob", wl)
        assert we[1] <= 1.0, (name, "entropy", we)
    assert sel_worst[1] <= 1.0, sel_worst
    assert agree <= 1.0, agree
    # the planted rows, by name (the per-row check above already holds them to fp64)
    for m, kind in c["plants"].items():
        if kind == "flat":
            assert abs(lp0[m].item() + math.log(512)) < 1e-6 and abs(en0[m].item() - math.log(512)) < 1e-6
        elif kind == "anti":
            assert abs(lp0[m].item() + 64) < 1e-4
        elif kind == "dominant" and (K >= 256 or int(tgt[m]) not in RL.TIE_COLS):
            assert -1e-3 < lp0[m].item() <= 0 and 0 <= en0[m].item() < 1e-2


def test_scoring_tail_targets_outside_the_vocabulary(ops):
    """Targets -1, 512, -7 and 2^32 + 7 (which a 32-bit compare would read as column 7): log-prob exactly 0 at those rows, every other
    row and every entropy bit for bit as without them -- in the fused tail and the profile launch, which take any int64; the
    two-kernel binding takes the negative ones (0) and REFUSES ids >= 512 (IndexError), and its kernel returns 0 for them when the
    binding's check is off."""
    M, K = 65, 288
    c = RL.exact_logit_case(M, K)
    hid, emb = c["hidden"].to(DEV), c["emb"].to(DEV)
    tgt = c["target"].clone()
    bad = {2: -1, 20: 512, 40: -7, 64: 2 ** 32 + 7}
    clean = c["target"].clone().to(DEV)
    for m, v in bad.items():
        tgt[m] = v
    tgt = tgt.to(DEV)
    keep = torch.ones(M, dtype=torch.bool, device=DEV)
    keep[list(bad)] = False
    lp0, en0 = ops.unembed_logprob(hid, emb, clean, want_logprob=True, want_entropy=True)
    lp, en = ops.unembed_logprob(hid, emb, tgt, want_logprob=True, want_entropy=True)
    _, lp_p, en_p = ops.unembed_profile(hid, emb, (7, 0), tgt)
    for got_lp, got_en in ((lp, en), (lp_p, en_p)):
        assert got_lp[list(bad)].tolist() == [0.0] * 4
        assert torch.equal(got_lp[keep], lp0[keep]) and torch.equal(got_en, en0)
    assert lp0[64].item() != 0.0                                            # (the row's in-range target has a log-prob to lose)
    logits = ops.linear(hid, emb, None)
    neg = clean.clone()
    neg[2], neg[40] = -1, -7
    lp2, en2 = ops.logprob_entropy(logits, neg, want_logprob=True, want_entropy=True)
    lp2c, _ = ops.logprob_entropy(logits, clean, want_logprob=True, want_entropy=True)
    assert lp2[2].item() == 0.0 and lp2[40].item() == 0.0
    k2 = torch.ones(M, dtype=torch.bool, device=DEV)
    k2[[2, 40]] = False
    assert torch.equal(lp2[k2], lp2c[k2])
    for v in (512, 2 ** 32 + 7):
        t = clean.clone()
        t[20] = v
        with pytest.raises(IndexError):
            ops.logprob_entropy(logits, t)
    was = ops.validate_ids
    try:
        ops.validate_ids = False                                           # the kernel's own 64-bit range check
        for lgts in (logits, logits.float()):
            lp3, _ = ops.logprob_entropy(lgts, tgt, want_logprob=True, want_entropy=True)
            assert lp3[list(bad)].tolist() == [0.0] * 4
    finally:
        ops.validate_ids = was


# =========================================================================================== 2. GELU gate on every finite bf16 input
def _gelu_report(tag, got, g):
    I = g.shape[1] // 2
    ratio, worst, bad = RL.gelu_gate_check(got, g)
    u = g[:, :I].reshape(-1)[worst].item()
    w = g[:, I:].reshape(-1)[worst].item()
    print(f"[rowlocal gelu {tag}] worst err / bound {ratio:.3f} at u = {u!r}, w = {w!r}; {int(bad.sum())} of {bad.numel()} outside")
    return ratio, int(bad.sum())


@pytest.mark.parametrize("gate", [1, -1, 2.0 ** -10, 30, "randn"])
@pytest.mark.parametrize("I", [8, 1032, 10928])
def test_gelu_gate_every_finite_bf16_input_vs_fp64(ops, I, gate):
    """u = all 65,280 finite bf16 patterns (+-0, subnormals, +-3.4e38) against gates 1, -1, 2^-10, 30 and a seeded randn, laid out as
    [M, 2 I]: I = 8 (one vector per row, 8,160 rows), 1032 (ivec = 129: a second block with ONE live thread), 10928 (the model's).
    Reference fp64 0.5 u (1 + erf(u / sqrt 2)) w; per-element bound 2^-8 |ref| + 0.5 |u| |w| (4.2e-7 + 2^-22) -- one bf16 rounding plus
    csrc/common.h's documented erf error and fp32 arithmetic carried through the product -- + 2^-134 where the rounding is a bf16
    subnormal's (rowlocal_ref.gelu_gate_bound); no tensor-wide term: the clamp at +-4, the negative tail where 1 + erf is of the size
    of the approximation's error, and every small output are judged on their own scale."""
    g = RL.gelu_inputs(I, gate).to(DEV)
    got = ops.gelu_gate(g)
    assert got.shape == (g.shape[0], I)
    ratio, n_bad = _gelu_report(f"I={I} gate={gate}", got, g)
    assert n_bad == 0 and ratio <= 1.0


def test_gelu_gate_rows_past_the_grid_cap(ops):
    """M = 16,389 > gridDim.y = 16,384 at I = 8: rows 16,384 .. 16,388 are the second pass of the row stride."""
    g = RL.gelu_inputs(8, "randn", M=16389, seed=3).to(DEV)
    got = ops.gelu_gate(g)
    ratio, n_bad = _gelu_report("M=16389 I=8", got, g)
    assert n_bad == 0 and ratio <= 1.0
    _, _, bad_tail = RL.gelu_gate_check(got[16384:], g[16384:])
    assert int(bad_tail.sum()) == 0 and bool((got[16384:].float().abs().sum(-1) > 0).any())


def test_gelu_gate_non_finite_inputs_stay_in_their_element(ops):
    """NaN, +inf and -inf among the u of a row (even and odd slots of the packed pairs, first and last vector): every OTHER element of
    the row stays inside the bound."""
    I = 1032
    g = RL.gelu_inputs(I, "randn", seed=4)
    for m in range(g.shape[0]):
        for j, v in ((0, float("nan")), (1, float("inf")), (13, float("-inf")), (514, float("nan")), (I - 1, float("inf")),
                     (I - 2, float("-inf")), (3 + 8 * (m % 100), float("nan"))):
            g[m, j] = v
    g = g.to(DEV)
    got = ops.gelu_gate(g)
    ratio, n_bad = _gelu_report("non-finite u, neighbours", got, g)          # (gelu_gate_check judges the finite u only)
    assert n_bad == 0 and ratio <= 1.0
    finite_u = torch.isfinite(g[:, :I].float())
    assert int((~finite_u).sum()) >= 6 * g.shape[0]
    assert bool(torch.isfinite(got.float()[finite_u & (g[:, :I].float().abs() < 1e30)]).all())


# =========================================================================================== 3. RMSNorm and its factor kernel
EPS = 1e-6


def _rms_case(ops, x, scale, bias):
    """One launch of ops.rmsnorm (+ ops.rms_finalize's tail-row path on the updated rows): (worst err / bound of the norm, worst rel err
    of the factor); the bias form's in-place row must be bf16(x + bias) bit for bit."""
    xd = x.to(DEV).clone()
    sd = scale.to(DEV)
    bd = bias.to(DEV) if bias is not None else None
    xn, ref = RL.rmsnorm64(x.to(DEV), sd, EPS, bd)
    out = ops.rmsnorm(xd, bd, sd, EPS)
    assert torch.equal(xd.view(torch.int16), xn.view(torch.int16))           # in place: bf16(x + bias), or untouched
    err = (out.double() - ref).abs()
    assert bool(torch.isfinite(out.float()).all())
    ratio = float((err / RL.rmsnorm_bound(ref)).max())
    rstd = ops.rms_finalize(None, xd, 0, EPS)[:x.shape[0]]
    r64 = RL.rstd64(xn, EPS)
    rel = float(((rstd.double() - r64).abs() / r64).max())
    return ratio, rel


@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("D", [8, 264, 1024, 1032, 4096, 4104, 8192])
def test_rmsnorm_element_bound_vs_fp64(ops, D, with_bias):
    """rmsnorm_kernel<*, 2> (D <= 1024), <*, 8> (<= 4096) and rmsnorm_long_kernel at both edges of each and with nvec % 64 != 0
    (8 -> nvec 1, 264 -> 33, 1032 -> 129, 4104 -> 513: the `idx < nvec` guard turns false inside a wave), 37 rows (a ragged last
    block), six input regimes: randn, randn x 2^+-40, one channel at 10^4 x the rest, a zero row, a row of bf16 subnormals.  Every
    element against gpu_ref64.rmsnorm64: |err| <= 2^-8 |ref| + 2^-21 |ref| + 2^-133 (one output rounding, fp32 arithmetic, the smallest
    bf16 subnormal) -- an outlier channel does not widen the other channels' bound.  rms_finalize's tail-row path on the same rows:
    1 / (rms + eps) to 2e-6 (the pin of test_gpu_gemm.py)."""
    M = 37
    worst, worst_rel = (0.0, ""), (0.0, "")
    for regime in RL.RMS_REGIMES:
        x, scale = RL.rmsnorm_inputs(M, D, regime)
        bias = torch.randn(D, generator=torch.Generator().manual_seed(D)).to(torch.bfloat16) if with_bias else None
        if with_bias and regime in ("big", "small"):
            bias = (bias.double() * 2.0 ** (40 if regime == "big" else -40)).to(torch.bfloat16)
        ratio, rel = _rms_case(ops, x, scale, bias)
        worst, worst_rel = max(worst, (ratio, regime)), max(worst_rel, (rel, regime))
        assert ratio <= 1.0, (regime, ratio)
        assert rel < 2e-6, (regime, rel)
    print(f"[rowlocal rmsnorm D={D} bias={with_bias}] worst err / bound {worst[0]:.3f} ({worst[1]}); rms_finalize tail rows worst rel "
          f"err {worst_rel[0]:.2e} ({worst_rel[1]})")


def test_rmsnorm_rows_past_the_grid_cap(ops):
    """M = 65,541 rows at D = 256: 16,386 blocks of four rows against the 16,384-block cap -- the last rows are the second pass of the
    grid stride -- every element against fp64, and rms_finalize (which launches one block per four rows, uncapped) on the same rows."""
    x, scale = RL.rmsnorm_inputs(65541, 256, "randn", seed=1)
    ratio, rel = _rms_case(ops, x, scale, None)
    print(f"[rowlocal rmsnorm M=65541 D=256] worst err / bound {ratio:.3f}; rms_finalize worst rel err {rel:.2e}")
    assert ratio <= 1.0 and rel < 2e-6


def test_rmsnorm_rows_tail_form_at_an_odd_width_keeps_its_pad_rows(ops):
    """evo_rmsnorm_rows_bf16 at D = 4104 (rmsnorm_long_kernel, nvec = 513) on the TAIL form of z^T (3 x 513 tokens: 512 main tokens per
    row at b * 512 + t, the last token of each row compactly behind Mp): every row against fp64 at its z^T row, bit for bit the plain
    launch's row, and the 13 pad rows behind the tail rows -- pre-filled with a canary -- untouched."""
    B, T, D = 3, 513, 4104
    Tm, Tp, Mp, r = ops.zt_layout(B, T)
    assert (Tm, Tp, Mp, r) == (512, 512, 1536, 1)
    x, scale = RL.rmsnorm_inputs(B * T, D, "outlier", seed=2)
    xd, sd = x.to(DEV), scale.to(DEV)
    canary = -1.5 * 2.0 ** 100
    try:
        buf = ops._xpad_buffer(B, T, D, xd.device)
        buf.fill_(canary)
        out = ops.rmsnorm_rows(xd, sd, EPS, B, T)
        assert out.data_ptr() == buf.data_ptr() and out.shape == (Mp + 16, D)
        bb = torch.arange(B, device=DEV)[:, None].expand(B, T).reshape(-1)
        tt = torch.arange(T, device=DEV)[None, :].expand(B, T).reshape(-1)
        rows = torch.where(tt < Tm, bb * Tp + tt, Mp + bb * r + (tt - Tm))
        assert rows.unique().numel() == B * T and int(rows.max()) == Mp + B * r - 1
        got = out[rows]
        _, ref = RL.rmsnorm64(xd, sd, EPS)
        ratio = float(((got.double() - ref).abs() / RL.rmsnorm_bound(ref)).max())
        assert torch.equal(got, ops.rmsnorm(xd.clone(), None, sd, EPS))
        pad = torch.ones(Mp + 16, dtype=torch.bool, device=DEV)
        pad[rows] = False
        assert int(pad.sum()) == 13 and bool((out[pad] == canary).all())
        print(f"[rowlocal rmsnorm_rows 3x513 D=4104 tail form] worst err / bound {ratio:.3f}; 13 pad rows keep the canary")
        assert ratio <= 1.0
    finally:
        ops.release_workspaces()                                            # (the canary must not outlive the test: pad rows are zero by contract)


# =========================================================================================== 4. rotary
ROPE_SHAPES = [(1, 3, 32, 128), (2, 5, 3, 16), (2, 32771, 1, 16)]


@pytest.mark.parametrize("B,T,H,hd", ROPE_SHAPES)
def test_rope_quarter_turn_tables_permute_exactly(ops, B, T, H, hd):
    """Tables with entries in {0, +-1} and q_scale a power of two: the output is an exact signed permutation of the input (q rows times
    the factor), compared BIT FOR BIT -- which row, which pair, which table row (t = n % T under the grid stride at 65,542 tokens), q
    against k rows, both passes of the `j` loop at H = 32, hd = 128 (per_tok = 512)."""
    qkv = torch.randn(B, T, 3, H, hd, generator=torch.Generator().manual_seed(T)).to(torch.bfloat16).to(DEV)
    cos, sin = RL.rope_table_pm1(T, hd)
    for qs in (1.0, 0.25):
        ref, _ = RL.rope64(qkv, cos.to(DEV), sin.to(DEV), q_scale=qs)
        got = ops.rope_(qkv.clone(), cos.to(DEV), sin.to(DEV), q_scale=qs)
        assert torch.equal(got.view(torch.int16), ref.to(torch.bfloat16).view(torch.int16))
        assert torch.equal(got[:, :, 2], qkv[:, :, 2])


@pytest.mark.parametrize("B,T,H,hd", ROPE_SHAPES)
def test_rope_element_bound_vs_fp64(ops, B, T, H, hd):
    """The model's table (bf16-rounded cos / sin of the fp32 angles, positions / 16 like the 131k yml), plain and with the attention's
    q_scale: every element against fp64 on that table, |err| <= 2^-8 |ref| + 2^-23 (|x0| + |x1|); V bit for bit untouched."""
    qkv = torch.randn(B, T, 3, H, hd, generator=torch.Generator().manual_seed(T + 1)).to(torch.bfloat16).to(DEV)
    cos, sin = (t.to(DEV) for t in RL.rope_table(T, hd, scaling=16.0))
    worst = 0.0
    for qs in (1.0, ops.attn_q_scale(hd)):
        ref, mag = RL.rope64(qkv, cos, sin, q_scale=qs)
        got = ops.rope_(qkv.clone(), cos, sin, q_scale=qs)
        assert torch.equal(got[:, :, 2].view(torch.int16), qkv[:, :, 2].view(torch.int16))
        ratio = float(((got.double() - ref).abs()[:, :, :2] / RL.rope_bound(ref, mag)[:, :, :2]).max())
        worst = max(worst, ratio)
        assert ratio <= 1.0, (qs, ratio)
    print(f"[rowlocal rope B={B} T={T} H={H} hd={hd}] worst err / bound {worst:.3f}")
