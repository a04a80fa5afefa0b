"""CPU: pins tests/rowlocal_ref.py -- the constructors' invariants and the fp64 references of tests/test_gpu_rowlocal.py -- where no GPU
is needed: the exact-logit constructor really is exact, the target rule covers every column in both halves, the planted rows have
the values their names promise, and every reference equals the oracle's operator (oracle/stripedhyena_ref.py) to 1e-12."""
import math

import pytest
import torch

import rowlocal_ref as RL
from oracle import stripedhyena_ref as R


@pytest.mark.parametrize("M,K", [(65, 32), (65, 288), (1061, 4096)])
def test_exact_logit_constructor_invariants(M, K):
    c = RL.exact_logit_case(M, K)
    hid, emb, tgt = c["hidden"], c["emb"], c["target"]
    assert hid.dtype == emb.dtype == torch.bfloat16 and hid.shape == (M, K) and emb.shape == (512, K)
    assert torch.equal(hid.double(), hid.double().round()) and float(hid.double().abs().max()) <= 4
    nnz = min(64, K)
    assert bool(((emb != 0).sum(-1) == nnz).all())                          # 64 nonzeros per row (32 at K = 32) ...
    assert bool((emb.double().abs()[emb != 0] == 2.0 ** -3 * (64 // nnz)).all())   # ... each +-2^-3 (+-2^-2 at K = 32)
    lg = RL.logits64(hid, emb)
    assert torch.equal(lg * 8, (lg * 8).round()) and float(lg.abs().max()) <= 32    # multiples of 1/8 inside +-32
    assert torch.equal(lg.to(torch.bfloat16).double(), lg)                  # exact in bf16
    assert torch.equal((hid.float() @ emb.float().t()).double(), lg)        # fp32 mm is exact on them
    assert torch.equal((hid.float().flip(-1) @ emb.float().flip(-1).t()).double(), lg)   # ... in another summation order too
    assert torch.equal(emb[RL.ANTI_C], -emb[RL.ANTI_T])
    # the planted rows
    lp, ent, _ = RL.logprob_entropy64(lg, tgt)
    kinds = {}
    for m, kind in c["plants"].items():
        kinds.setdefault(kind, []).append(m)
        row = lg[m]
        if kind == "dominant":
            assert float(row[tgt[m]]) == 32.0 == float(row.max())
            if K >= 256 or int(tgt[m]) not in RL.TIE_COLS:
                assert -1e-3 < float(lp[m]) <= 0 and float(ent[m]) < 1e-2
        elif kind == "flat":
            assert bool((row == 0).all())
            assert abs(float(lp[m]) + math.log(512)) < 1e-12 and abs(float(ent[m]) - math.log(512)) < 1e-12
        elif kind == "tie":
            assert [float(row[n]) for n in RL.TIE_COLS] == [32.0] * 4 == [float(row.max())] * 4
        elif kind == "anti":
            assert int(tgt[m]) == RL.ANTI_T and float(row[RL.ANTI_T]) == -32.0 and float(row[RL.ANTI_C]) == 32.0 == float(row.max())
            assert abs(float(lp[m]) + 64) < 1e-3
    assert {k: len(v) for k, v in kinds.items()} == {"dominant": 16, "flat": 2, "tie": 2, "anti": 2}
    # the row maximum of the dominant rows visits every (wave, lane half) in both 32-row halves of the workgroup
    seen = {(RL.half_index(m)[1], int(tgt[m]) >> 7, (int(tgt[m]) >> 2) & 1) for m in kinds["dominant"]}
    assert seen == {(h, w, l) for h in (0, 1) for w in range(4) for l in (0, 1)}


def test_target_rule_covers_every_column_in_both_halves_at_1061_rows():
    cov = RL.target_coverage(RL.exact_targets(1061))
    assert cov.shape == (2, 512) and int(cov.min()) >= 1
    assert int(RL.target_coverage(RL.exact_targets(1023)).min()) == 0       # (and the count sees a hole: 1,023 rows cannot cover)
    tg = RL.exact_targets(65)
    tg[3] = -1
    tg[5] = 2 ** 32 + 7
    assert int(RL.target_coverage(tg).sum()) == 63


def test_logprob_references_equal_the_oracle():
    g = torch.Generator().manual_seed(3)
    lg = (torch.randn(37, 512, generator=g) * 4).double()
    tg = torch.randint(0, 512, (37,), generator=g)
    tg[4] = -1
    lp, ent, sl = RL.logprob_entropy64(lg, tg, sel=(3, 500))
    rlp, rent = R.op_logprob_entropy(lg, tg)
    assert float((lp - rlp).abs().max()) <= 1e-12 and float((ent - rent).abs().max()) <= 1e-12 and float(lp[4]) == 0.0
    assert torch.equal(sl, torch.log_softmax(lg, -1)[:, [3, 500]])
    tg2 = tg.clone()
    tg2[0], tg2[1], tg2[2] = 512, -7, 2 ** 32 + 7
    lp2, _, _ = RL.logprob_entropy64(lg, tg2)
    assert lp2[:3].tolist() == [0.0, 0.0, 0.0] and torch.equal(lp2[3:], lp[3:])
    # the fp32 restatement is the same function: close to fp64 at fp32's precision, and its allowance is 4 x its own error with a floor
    lp32, ent32, sl32 = RL.logprob_entropy_f32(lg, tg, sel=(3, 500))
    assert lp32.dtype == torch.float32 and float((lp32.double() - lp).abs().max()) < 2e-5
    assert float((ent32.double() - ent).abs().max()) < 2e-5 and float((sl32.double() - sl).abs().max()) < 2e-5
    allow, e32 = RL.measured_allowance(lp, lp32)
    assert e32 == float((lp32.double() - lp).abs().max())
    assert bool((allow >= 4 * e32).all()) and bool((allow >= 2.0 ** -22 * (1 + lp.abs())).all())
    assert bool((allow <= torch.clamp(2.0 ** -22 * (1 + lp.abs()), min=4 * e32)).all())


def test_gelu_inputs_and_reference():
    u = RL.all_finite_bf16()
    assert u.numel() == 65280 and bool(torch.isfinite(u.float()).all())
    assert u.view(torch.int16).unique().numel() == 65280                    # every pattern once: +-0 and the subnormals included
    assert int((u.float() == 0).sum()) == 2 and int(((u.float() != 0) & (u.float().abs() < 2.0 ** -126)).sum()) == 254
    for I in (8, 1032, 10928):
        g = RL.gelu_inputs(I, 30)
        assert g.shape[1] == 2 * I and g.shape[0] * I >= 65280 and (g.shape[0] - 1) * I < 65280
        assert g[:, :I].reshape(-1)[:65280].view(torch.int16).unique().numel() == 65280
        assert bool((g[:, I:] == 30).all())
    assert (1032 // 8 + 127) // 128 == 2 and 1032 // 8 - 128 == 1           # ivec = 129: a second block with one live thread
    g = torch.randn(9, 64, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16)
    assert float((RL.gelu_gate64(g) - R.op_gelu_gate(g)).abs().max()) <= 1e-12
    # the bound has no tensor-wide term: it scales with the element
    g2 = torch.tensor([[1.0, 2.0 ** -100, 3.0, 5.0]], dtype=torch.bfloat16)
    b = RL.gelu_gate_bound(g2, RL.gelu_gate64(g2))
    assert float(b[0, 1]) < 2.0 ** -105 and float(b[0, 0]) > 2.0 ** -10
    # the checker: an exact output passes, one bf16 ulp off fails, the right infinity beyond the bf16 range passes
    ref = RL.gelu_gate64(g)
    assert RL.gelu_gate_check(ref.to(torch.bfloat16), g)[0] <= 1.0
    off = (ref.to(torch.bfloat16).view(torch.int16) + 1).view(torch.bfloat16)
    assert RL.gelu_gate_check(off, g)[0] > 1.0
    big = torch.tensor([[3.0e38, -3.0e38, 30.0, 30.0]], dtype=torch.bfloat16)
    assert RL.gelu_gate_check(torch.tensor([[float("inf"), 0.0]], dtype=torch.bfloat16), big)[0] <= 1.0
    assert RL.gelu_gate_check(torch.tensor([[float("-inf"), 0.0]], dtype=torch.bfloat16), big)[0] > 1.0


@pytest.mark.parametrize("regime", RL.RMS_REGIMES)
@pytest.mark.parametrize("with_bias", [False, True])
def test_rmsnorm_reference_equals_the_oracle(regime, with_bias):
    x, scale = RL.rmsnorm_inputs(9, 264, regime)
    bias = torch.randn(264, generator=torch.Generator().manual_seed(1)).to(torch.bfloat16) if with_bias else None
    xn, ref = RL.rmsnorm64(x, scale, 1e-6, bias)
    rx, rref = R.op_rmsnorm(xn, scale, 1e-6)
    assert float(((ref - rref).abs() / (1 + rref.abs())).max()) <= 1e-12
    if with_bias:
        assert torch.equal(xn, (x.float() + bias.float()).to(torch.bfloat16))
        assert float(((R.op_rmsnorm(x, scale, 1e-6, bias)[0] - xn.double()).abs() / (2.0 ** -8 * xn.double().abs() + 2.0 ** -133)).max()) <= 1
    else:
        assert xn is x
    r = RL.rstd64(xn, 1e-6)
    assert float((r[:, None] * xn.double() * scale.double() - ref).abs().max()) <= 1e-12 * float(1 + ref.abs().max())
    if regime == "zero_row" and not with_bias:
        assert bool((ref[4] == 0).all()) and abs(float(r[4]) - 1e6) < 1e-6
    if regime == "subnormal_row" and not with_bias:
        assert float(xn[4].double().abs().max()) < 2.0 ** -126 and float(xn[4].double().abs().max()) > 0


def test_rope_reference_equals_the_oracle_and_quarter_turns_permute():
    g = torch.Generator().manual_seed(2)
    qkv = torch.randn(2, 5, 3, 3, 16, generator=g).to(torch.bfloat16)
    cos, sin = RL.rope_table(5, 16, scaling=16.0)
    assert torch.equal(cos, cos.bfloat16().float())
    out, mag = RL.rope64(qkv, cos, sin)
    assert float((out - R.op_rope(qkv, cos, sin)).abs().max()) <= 1e-12
    assert torch.equal(out[:, :, 2], qkv[:, :, 2].double()) and bool((mag[:, :, 2] == 0).all())
    out_s, _ = RL.rope64(qkv, cos, sin, q_scale=0.3)
    qs = float(torch.tensor(0.3, dtype=torch.float32))
    assert torch.equal(out_s[:, :, 0], out[:, :, 0] * qs) and torch.equal(out_s[:, :, 1:], out[:, :, 1:])
    # quarter turns: entries in {0, +-1}, the output a signed permutation of the input (exact in bf16 with a power-of-two factor)
    c1, s1 = RL.rope_table_pm1(5, 16)
    assert set(c1.unique().tolist()) <= {-1.0, 0.0, 1.0} and bool((c1.abs() + s1.abs() == 1).all())
    o1, _ = RL.rope64(qkv, c1, s1, q_scale=0.25)
    assert torch.equal(o1.to(torch.bfloat16).double(), o1)
    for w, f in ((0, 0.25), (1, 1.0)):
        a = o1[:, :, w].abs().reshape(10, 3, 2, 8).sort(dim=2).values
        b = (qkv[:, :, w].double().abs() * f).reshape(10, 3, 2, 8).sort(dim=2).values
        assert torch.equal(a, b)
