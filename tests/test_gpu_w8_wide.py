"""GPU (-m gpu): FP8 (e4m3fn) weights of the decode step at 9-64 rows -- the MFMA weight-streaming forms of csrc/skinny_fp8.hip
(evo_linear_skinny_w8, evo_mlp_gate_skinny_w8; DESIGN.md section 28, tests/PARITY_w8_wide.md).

  * both entries on EXACT sums (both designs of tests/w8_ref.py, both x units): the output equals dense_exact.expected(...) on the
    dequantised weight bit for bit, whatever partition of K the launch chose; the gate by row 24b's bound on g = [bf16(S1) | bf16(S2)],
    as tests/test_gpu_w8.py judges the 1-8-row forms.  M on both sides of every m-tile boundary; N ragged, K one chunk, K = 11,008
    (43 units of 256 over the slices);
  * random data against fp64 on the dequantised weight under the bounds tests/test_gpu_gemv.py applies to the bf16 entries;
  * both entries inside the arena (tests/arena.py);
  * the model: pools of 12 (toy) and 9 (d4096) slots and a generate() batch of 9 against the fp64 oracle holding the dequantised
    weights (row 23's rule), captured = eager, seeded runs repeat, bf16 untouched, 8 slots still on the dot2 launches, the combined case.

Instantiation -> the test that reaches it (MT = 1 .. 4 from M = 5 | 9 | 16, 17 | 32, 33 | 48, 49 | 64):
  skinny_w8_kernel<MT, 2>                 test_nsplit[8200-256 | 8200-1024], test_narrow_unsplit
  skinny_w8_kernel<MT, 3>                 test_nsplit[12288-4096]
  skinny_w8_kernel<MT, 4>                 test_random_linear[16640-512]
  skinny_w8_kernel<MT, 4, true> + reduce  test_splitk
  skinny_w8_kernel<MT, 4, false, true>    test_gate (both layouts)
"""
import pytest
import torch

import dense_exact as DX
import w8_ref as W8
import w8_wide_ref as WW
from evo_amd.sh.cache import Fp8Weight
from oracle import stripedhyena_ref as R
from test_gpu_arena import _run, covers, gen, is_poison, poisoned, rnd
from test_gpu_model import DEV, rel_l2
from test_gpu_pool import PROMPTS
from test_gpu_w8 import (MODES, N_TOK, THREE, _assert_logits_vs_oracle, _exact, _gate, _ops, _pool, _quantised, _rec_inputs, _Spans, _tok,
                         _twin)

pytestmark = pytest.mark.gpu
BF = torch.bfloat16
UNITS = pytest.mark.parametrize("unit", DX.X_UNITS, ids=["integers", "sixteenths"])
DESIGNS = pytest.mark.parametrize("design", list(W8.DESIGNS))


def _skinny(ops, x, rec, b=None, res=None, ws=None):
    """evo_linear_skinny_w8 called directly (any M in 5 .. 64, the caller's workspace or none), under the product's span."""
    M, K = x.shape
    N = rec.data.shape[0]
    y = res if res is not None else torch.empty(M, N, dtype=BF, device=x.device)
    ops._launch("skinny_w8", "evo_linear_skinny_w8", x.data_ptr(), rec.data.data_ptr(), rec.scale.data_ptr(), None if b is None else b.data_ptr(),
                None if res is None else res.data_ptr(), y.data_ptr(), M, N, K, None if ws is None else ws.data_ptr(),
                0 if ws is None else ws.numel() * 4)
    return y


def _linear_cases(ops, N, K, design, unit, Ms, call, what):
    """Every M of `Ms` x {plain, bias, residual, both}: bit for bit, twice, the residual aliasing y, 3 rows behind M keeping their bits."""
    w = W8.DESIGNS[design][0](N, K, device=DEV)
    rec, wd = _quantised(ops, w)
    assert torch.equal(DX.bits(wd), DX.bits(w)), "the design is not a fixed point of the rule"
    Mx = max(Ms)
    x, b, r = DX.make_x(Mx, K, device=DEV, unit=unit), DX.make_bias(N, device=DEV), DX.make_residual(Mx + 3, N, device=DEV)
    S = DX.exact_product(x, wd)
    for M in Ms:
        xm = x[:M].contiguous()
        for name, bias, res in MODES:
            want = DX.expected(xm, wd, b if bias else None, r[:M] if res else None, S=S[:M])

            def run():
                if not res:
                    return call(M, xm, rec, b if bias else None, None)
                buf = r.clone()
                out = call(M, xm, rec, b if bias else None, buf[:M])
                assert out.data_ptr() == buf.data_ptr() and torch.equal(DX.bits(buf[M:]), DX.bits(r[M:])), "rows behind M were written"
                return buf[:M]
            with _Spans(ops) as sp:
                got, again = run(), run()
            assert sp.count == {"skinny_w8": 2}, sp.count
            _exact(got, want, f"{what} {design} x/{unit} M={M} N={N} K={K} {name}")
            assert torch.equal(got, again)


def _public(ops):
    """The product's route: linear_w8 / linear_residual_w8_ from 9 rows on (they pick the workspace); the entry itself at 5 rows."""
    def call(M, xm, rec, b, res):
        if M <= 8:
            return _skinny(ops, xm, rec, b, res)
        return ops.linear_w8(xm, rec, b) if res is None else ops.linear_residual_w8_(res, xm, rec, bias=b)
    return call


# =============================================================================== exact sums: n-split, whole K per wave
@UNITS
@DESIGNS
@pytest.mark.parametrize("N,K", WW.NSPLIT)
def test_nsplit(N, K, design, unit):
    ops = _ops()
    _linear_cases(ops, N, K, design, unit, WW.NSPLIT_M, _public(ops), "skinny_w8 n-split")


# =============================================================================== exact sums: SPLITK + the slice reduction
@UNITS
@DESIGNS
@pytest.mark.parametrize("N,K", WW.SPLITK)
def test_splitk(N, K, design, unit):
    """The caller's workspace, poisoned: the launch wrote its slices * M * N partial sums there and nothing behind them."""
    ops = _ops()
    slices = WW.slices(N, K)
    assert slices >= 2
    ws = poisoned((8 * 64 * N + 64,), torch.float32)

    def call(M, xm, rec, b, res):
        ws.view(torch.int32).fill_(-1)
        y = _skinny(ops, xm, rec, b, res, ws=ws)
        used = ws[:slices * M * N].view(torch.int32)
        assert not bool((used == -1).any()) and is_poison(ws[slices * M * N:]), "the split over K did not run as stated"
        return y
    _linear_cases(ops, N, K, design, unit, WW.SPLITK_M, call, f"skinny_w8 SPLITK x{slices}")
    _linear_cases(ops, N, K, design, unit, (WW.SPLITK_M[0], WW.SPLITK_M[-1]), _public(ops), "skinny_w8 SPLITK (ops workspace)")


# =============================================================================== exact sums: narrow layers on the unsplit form
@UNITS
@DESIGNS
@pytest.mark.parametrize("N,K", WW.NARROW)
def test_narrow_unsplit(N, K, design, unit):
    """No workspace, or N % 64 != 0, or a single 256-k unit: the n-split form serves any N."""
    ops = _ops()
    _linear_cases(ops, N, K, design, unit, WW.NARROW_M, lambda M, xm, rec, b, res: _skinny(ops, xm, rec, b, res, ws=None), "skinny_w8 narrow")


# =============================================================================== exact sums: the gate
@UNITS
@DESIGNS
@pytest.mark.parametrize("I,K", WW.GATE)
def test_gate(I, K, design, unit):
    ops = _ops()
    w12 = W8.DESIGNS[design][1](I, K, device=DEV)
    assert torch.equal(DX.bits(ops.w_quant_fp8(w12).dequantize()), DX.bits(w12))
    x = DX.make_x(max(WW.GATE_M), K, device=DEV, unit=unit)
    S = DX.exact_product(x, w12)
    if K >= 4096:
        assert float(DX.gate_reference(S, I)[:, :I].double().std()) > 1.0      # u spans the GELU's curved range
    for lname, wsrc, grouped in (("plain", w12, False), ("grouped", ops.pack_gate_weights(w12), True)):
        rec = ops.w_quant_fp8(wsrc)
        for M in WW.GATE_M:
            xm = x[:M].contiguous()

            def run():
                if M > 8:
                    return ops.mlp_gate_w8(xm, rec, grouped=grouped)
                a = torch.empty(M, I, dtype=BF, device=DEV)
                ops._launch("skinny_gate_w8", "evo_mlp_gate_skinny_w8", xm.data_ptr(), rec.data.data_ptr(), rec.scale.data_ptr(), a.data_ptr(), M, I, K,
                            int(grouped))
                return a
            with _Spans(ops) as sp:
                got, again = run(), run()
            assert sp.count == {"skinny_gate_w8": 2}, sp.count
            _gate(got, DX.gate_reference(S[:M], I), f"skinny_gate_w8 {design} x/{unit} M={M} I={I} K={K} {lname}")
            assert torch.equal(got, again)


# =============================================================================== random data vs fp64 on the dequantised weights
@pytest.mark.parametrize("M", [9, 32, 64])
@pytest.mark.parametrize("N,K", [(12288, 4096), (4096, 11008), (16640, 512)])
@pytest.mark.parametrize("mode", ["plain", "bias", "residual"])
def test_random_linear(M, N, K, mode):
    ops = _ops()
    g = torch.Generator().manual_seed(M * 1000 + N + K)
    x = torch.randn(M, K, generator=g).bfloat16().to(DEV)
    rec = ops.w_quant_fp8((torch.randn(N, K, generator=g) * 0.05).bfloat16().to(DEV))
    b, r = torch.randn(N, generator=g).bfloat16().to(DEV), torch.randn(M, N, generator=g).bfloat16().to(DEV)
    ref = x.double() @ rec.dequantize().double().t()
    if mode == "bias":
        got, ref = ops.linear_w8(x, rec, b), ref + b.double()
    elif mode == "residual":
        got, ref = ops.linear_residual_w8_(r.clone(), x, rec), ref + r.double()
    else:
        got = ops.linear_w8(x, rec)
    err = (got.double() - ref).abs()
    assert (err <= ref.abs() * 2 ** -8 + 2e-3 * ref.abs().max()).all()          # tests/test_gpu_gemv.py:41
    assert ((got.double() - ref).norm() / ref.norm()).item() < 2e-3             # tests/test_gpu_gemv.py:42


@pytest.mark.parametrize("M", [9, 32, 64])
@pytest.mark.parametrize("norm", [True, False])
def test_random_gate(M, norm, I=11008, K=4096):
    """With the norm in front the product runs the norm pass and then the launch (the fold ends at 8 rows)."""
    ops = _ops()
    g = torch.Generator().manual_seed(M * 77 + I + K)
    x = (torch.randn(M, K, generator=g) * 2).bfloat16().to(DEV)
    scale = (1 + 0.1 * torch.randn(K, generator=g)).bfloat16().to(DEV)
    rec = ops.w_quant_fp8((torch.randn(2 * I, K, generator=g) * (1.5 / K ** 0.5)).bfloat16().to(DEV))
    wd = rec.dequantize().double()
    with _Spans(ops) as sp:
        got = ops.mlp_gate_w8(x, rec, scale, 1e-6) if norm else ops.mlp_gate_w8(x, rec)
    assert sp.count.get("skinny_gate_w8") == 1 and not any(k.startswith("gemv") for k in sp.count), sp.count
    xd = (ops.rmsnorm(x.clone(), None, scale, 1e-6) if norm else x).double()
    u, v = (xd @ wd[:I].t()).bfloat16().double(), (xd @ wd[I:].t()).bfloat16().double()
    want = torch.nn.functional.gelu(u) * v
    err = (got.double() - want).abs()
    assert bool((err <= want.abs() * 2.0 ** -6 + 2e-3 * want.abs().max()).all())   # tests/test_gpu_gemv.py:84 / :139
    assert ((got.double() - want).norm() / want.norm()).item() < 4e-3              # tests/test_gpu_gemv.py:85 / :140


# =============================================================================== the arena
@covers("evo_linear_skinny_w8")
@pytest.mark.parametrize("M,N,K", [(9, 4104, 256), (33, 4096, 4096)])
def test_arena_linear(M, N, K):
    """(33, 4096, 4096): the split over K, its workspace allocated inside the arena (release_workspaces drops it on the way out)."""
    ops = _ops()
    data, scale = _rec_inputs(N, K, None)
    inp = {"x": rnd((M, K), gen(M)), "data": data, "scale": scale, "b": rnd((N,), gen(2)), "res": rnd((M + 2, N), gen(3))}
    _run(lambda x, data, scale, b, res: ops.linear_residual_w8_(res[:M], x, Fp8Weight(data, scale), bias=b), inp, inout=["res"],
         expect=["evo_linear_skinny_w8"], align={"scale": 4})
    _run(lambda x, data, scale, b, res: ops.linear_w8(x, Fp8Weight(data, scale)), inp, expect=["evo_linear_skinny_w8"], align={"scale": 4})


@covers("evo_mlp_gate_skinny_w8")
@pytest.mark.parametrize("M,I,K,grouped", [(17, 64, 256, True), (9, 64, 512, False)])
def test_arena_gate(M, I, K, grouped):
    ops = _ops()
    data, scale = _rec_inputs(2 * I, K, None)
    inp = {"x": rnd((M, K), gen(M)), "data": data, "scale": scale}
    _run(lambda x, data, scale: ops.mlp_gate_w8(x, Fp8Weight(data, scale), grouped=grouped), inp, expect=["evo_mlp_gate_skinny_w8"],
         align={"scale": 4})


# =============================================================================== the model
TWELVE = THREE + [p for p in PROMPTS if p not in THREE] + ["ACGTTGCAAC", "TTGACA" * 7, "GGGCCCAAATTT" * 3, "CATG" * 9, "A" * 17, "TGCA" * 21]
NEW_SPANS = ("skinny_w8", "skinny_gate_w8")


def _fp8_pool_runs(m, n_slots, prompts, seed=11):
    """{captured?: (ids, logits)} of a seeded FP8 pool, one sample per prompt; the eager run also proves which launches a step makes."""
    runs = {}
    for graph in (True, False):
        pool = _pool(m, use_graph=graph, n_slots=n_slots, seed=seed, weight_dtype="fp8")
        with _Spans(m.ops) as sp:
            pool.generate(prompts, n_tokens=N_TOK, n_sample_per_prompt=1)
        assert pool.stats["weight_dtype"] == "fp8" and pool.stats["decode_weight_bytes"] == m.decode_weight_bytes("fp8")
        if not graph:
            assert all(sp.count.get(k, 0) > 0 for k in NEW_SPANS) and not any(k.startswith("gemv") and k.endswith("_w8") for k in sp.count), sp.count
        runs[graph] = (pool.last_ids.clone(), pool.last_logits.clone())
    assert torch.equal(runs[True][0], runs[False][0]) and torch.equal(runs[True][1], runs[False][1]), "captured step != eager step"
    return runs[True]


def test_toy_pool_of_12_slots_vs_the_fp64_oracle():
    """12 streams x 24 tokens, every slot busy from the first step; row 23's rule as tests/test_gpu_w8.py:480 applies it, on THREE."""
    cfg, sd, m = _twin("toy")
    assert len(TWELVE) == 12 and len(set(TWELVE)) == 12
    ids, logits = _fp8_pool_runs(m, 12, TWELVE)
    _assert_logits_vs_oracle("w8 pool toy, 12 slots", cfg, sd, None, ids, logits)


def test_d4096_pool_of_9_slots_vs_the_fp64_oracle():
    cfg, sd, m = _twin("d4096")
    ids, logits = _fp8_pool_runs(m, 9, TWELVE[:9])
    _assert_logits_vs_oracle("w8 pool d4096, 9 slots", cfg, sd, DEV, ids, logits)


def test_generate_with_9_prompts_vs_the_fp64_oracle():
    """Generator.generate on a batch of 9 equal-length prompts: the prefill reads the bf16 weights, the steps the FP8 set (the same
    values on this model); three rows against the oracle under the criterion of tests/test_gpu_w8.py:480."""
    from evo_amd.generation import Generator
    cfg, sd, m = _twin("toy")
    prompts = [(p * 32)[:32] for p in TWELVE[:9]]
    ids = torch.tensor([list(p.encode()) for p in prompts], device=DEV)
    g = Generator(m, _tok(), top_k=1, top_p=1.0, temperature=0.0, weight_dtype="fp8")
    with _Spans(m.ops) as sp:
        out, logits, _ = g.generate(DEV, input_ids=ids, num_tokens=N_TOK, cached_generation=True, print_generation=False, stop_at_eos=False)
    assert all(sp.count.get(k, 0) > 0 for k in NEW_SPANS), sp.count
    oracle, oracle_bf16 = R.RefStripedHyena(cfg, sd, "fp64"), R.RefStripedHyena(cfg, sd, "bf16")
    worst = floor = 0.0
    for j in (0, 4, 8):
        full = torch.cat([ids[j: j + 1], out[j: j + 1]], dim=1).cpu()
        P = ids.shape[1]
        ref = oracle(full)[0][0][P - 1: P - 1 + N_TOK]
        worst = max(worst, rel_l2(logits[j].cpu(), ref))
        floor = max(floor, rel_l2(oracle_bf16(full)[0][0][P - 1: P - 1 + N_TOK], ref))
    print(f"[w8 generate, 9 prompts] logits vs the fp64 oracle on the dequantised weights: worst rel-L2 {worst:.3e} (eager-bf16 oracle {floor:.3e})")
    assert worst < max(1.5 * floor, 4e-3), (worst, floor)                # tests/test_gpu_w8.py:480


def test_seeded_12_slot_runs_repeat_and_bf16_is_untouched():
    _, _, m = _twin("toy")

    def run(**kw):
        pool = _pool(m, n_slots=12, seed=5, **kw)
        pool.generate(TWELVE, n_tokens=N_TOK, n_sample_per_prompt=1)
        return pool.last_ids.clone(), pool.last_logits.clone()
    before = run()
    a, b = run(weight_dtype="fp8"), run(weight_dtype="fp8")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    after = run()
    assert torch.equal(before[0], after[0]) and torch.equal(before[1], after[1])


def test_8_slots_stay_on_the_dot2_launches():
    """The routing at <= 8 rows did not move: an 8-slot FP8 pool makes gemv_*_w8 launches only, captured = eager."""
    _, _, m = _twin("toy")
    runs = {}
    for graph in (True, False):
        pool = _pool(m, use_graph=graph, n_slots=8, seed=11, weight_dtype="fp8")
        with _Spans(m.ops) as sp:
            pool.generate(TWELVE[:8], n_tokens=N_TOK, n_sample_per_prompt=1)
        if not graph:
            assert not any(k in sp.count for k in NEW_SPANS), sp.count
            assert {"gemv_w8", "gemv_gate_w8"} <= set(sp.count), sp.count
        runs[graph] = (pool.last_ids.clone(), pool.last_logits.clone())
    assert torch.equal(runs[True][0], runs[False][0]) and torch.equal(runs[True][1], runs[False][1])
    ops = _ops()
    rec = ops.w_quant_fp8(W8.make_w4(4096, 512, device=DEV))
    with _Spans(ops) as sp:
        ops.linear_w8(DX.make_x(8, 512, device=DEV), rec)
        ops.mlp_gate_w8(DX.make_x(8, 512, device=DEV), rec)
    assert sp.count == {"gemv_w8": 1, "gemv_gate_w8": 1}, sp.count


def test_combined_case_at_12_slots():
    _, _, m = _twin("toy")
    pool = _pool(m, n_slots=12, seed=3, weight_dtype="fp8", kv_dtype="fp8", allowed_tokens="ACGT")
    seqs, scores, owner = pool.generate(TWELVE, n_tokens=N_TOK, n_sample_per_prompt=2, stop_sequences=["TAA", "TAG", "TGA"], stop_frame=3,
                                        return_logits=False)
    assert len(seqs) == 24 and all(set(s) <= set("ACGT") and 1 <= len(s) <= N_TOK for s in seqs)
    assert pool.stats["weight_dtype"] == "fp8" and pool.stats["decode_weight_bytes"] == m.decode_weight_bytes("fp8")
    assert pool.stats["stop_ends"] + pool.stats["length_ends"] == len(seqs)
