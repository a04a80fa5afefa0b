"""GPU (-m gpu): the decode pool's opt-in batch-invariant step.  With `batch_invariant=True` a job's tokens, recorded
logits and `last_logprobs` are the same BITS at any slot count, in any slot, beside any other jobs, at any cache capacity, paged or not,
captured or eager.  Without the option none of this holds (tests/test_gpu_pool.py's docstring): the dense launches pick a form per row count
and the decode attention a split count per capacity, and every form sums in another order.

The toy model of the other pool tests (D = 512: every dense layer of its step meets the row-invariant launches' contract), eight prompts
of 5 to 70 tokens: with 12 tokens each the capacity stays far below the 1,857 keys from which the default split count stops changing."""
import numpy as np
import pytest
import torch

from oracle import stripedhyena_ref as R
from test_gpu_model import DEV, SMALL4, build, rel_l2

pytestmark = pytest.mark.gpu

LENGTHS = [5, 70, 13, 64, 31, 9, 47, 22]
N_TOK, SEED = 12, 7


def _prompt(n, seed):
    return "".join(np.random.default_rng(seed).choice(list("ACGT"), size=n))


PROMPTS = [_prompt(n, 100 + i) for i, n in enumerate(LENGTHS)]
LONG = _prompt(600, 99)


@pytest.fixture(scope="module")
def toy():
    from evo_amd.tokenizer import CharLevelTokenizer
    cfg, sd, m = build(dict(SMALL4, use_interpolated_rotary_pos_emb=True, rotary_emb_scaling_factor=16))
    return cfg, sd, m, CharLevelTokenizer(512)


def _run(toy, n_slots, prompts=PROMPTS, n_tokens=None, streams=None, batch_invariant=True, pool_kw=None, **gen):
    """One pool call on the job-control path (per-prompt limits: it records `last_logprobs`) -> {prompt: (ids, logits, logprobs, string)}."""
    from evo_amd.pool import DecodePool
    _, _, m, tok = toy
    pool = DecodePool(m, tok, n_slots=n_slots, top_k=4, top_p=1.0, temperature=1.0, device=DEV, seed=SEED, allowed_tokens="ACGT",
                      batch_invariant=batch_invariant, **(pool_kw or {}))
    n_tokens = [N_TOK] * len(prompts) if n_tokens is None else n_tokens
    seqs, scores, owner = pool.generate(prompts, n_tokens=n_tokens, streams=streams, **gen)
    assert owner == list(range(len(prompts))) and pool.stats["batch_invariant"] is batch_invariant
    return {p: (pool.last_ids[j].clone(), pool.last_logits[j].clone(), pool.last_logprobs[j].clone(), seqs[j], pool.last_lengths[j])
            for j, p in enumerate(prompts)}


def _same(got, want, what, prompts=PROMPTS):
    for p in prompts:
        n = want[p][4]
        assert got[p][4] == n and got[p][3] == want[p][3], f"{what}: the job of the {len(p)}-token prompt generated another string"
        for k, name in enumerate(("ids", "recorded logits", "last_logprobs")):
            assert torch.equal(got[p][k][:n], want[p][k][:n]), f"{what}: {name} of the {len(p)}-token prompt's job differ"


@pytest.fixture(scope="module")
def reference(toy):
    return _run(toy, 8)


@pytest.mark.parametrize("n_slots", [1, 3, 9, 17, 33])
def test_any_slot_count(toy, reference, n_slots):
    _same(_run(toy, n_slots), reference, f"{n_slots} slots against 8")


def test_any_order_any_company_any_capacity(toy, reference):
    n = len(PROMPTS)
    _same(_run(toy, 3, prompts=PROMPTS[::-1], streams=list(range(n))[::-1]), reference, "prompts in reversed order")
    # one more job of 600 + 700 tokens: the capacity of the call goes from 82 keys to 1,300, the default split count from 4 to 24
    got = _run(toy, 4, prompts=PROMPTS + [LONG], n_tokens=[N_TOK] * n + [700])
    _same(got, reference, "beside a 600-token prompt with 700 tokens to go")
    assert got[LONG][4] == 700


def test_paged_and_eager(toy, reference, monkeypatch):
    _same(_run(toy, 3, pool_kw=dict(kv_paged=True, kv_page_tokens=64)), reference, "kv_paged, 64-token pages")
    monkeypatch.setenv("EVO_AMD_DECODE_GRAPH", "0")
    _same(_run(toy, 5, pool_kw=dict(use_graph=False)), reference, "eager launches")


def test_stop_rules_and_constraints(toy):
    import evo_amd
    for what, gen in (("a stop sequence", dict(stop_sequences=["TA", "GG"], stop_frame=2)),
                      ("an IUPAC template", dict(constraints=evo_amd.iupac_template("ATGNNRYNNTAA")))):
        a, b = _run(toy, 2, **gen), _run(toy, 9, **gen)
        _same(a, b, f"{what}, 2 slots against 9")
        if "constraints" in gen:
            assert all(a[p][4] == 12 and a[p][3].startswith("ATG") and a[p][3].endswith("TAA") for p in PROMPTS)
        else:
            assert any(a[p][4] < N_TOK for p in PROMPTS), "no job ended on the stop sequence: the rule was not exercised"


def test_a_default_pool_is_untouched_by_an_invariant_pool_on_the_same_model(toy, reference):
    before = _run(toy, 3, batch_invariant=False)
    _same(_run(toy, 3), reference, "between two default pools")
    after = _run(toy, 3, batch_invariant=False)
    _same(after, before, "the default pool, before and after an invariant pool")


def test_recorded_logits_against_the_fp64_oracle(toy, reference):
    """tests/test_gpu_pool.py's rule for the default bf16 step (tests/PARITY.md row 23): worst rel-L2 against the fp64 oracle on the very
    same tokens below 1.5 x the oracle's own eager-bf16 restatement (and never below 4e-3)."""
    from evo_amd.scoring import prepare_batch
    cfg, sd, m, tok = toy
    oracle, oracle_bf16 = R.RefStripedHyena(cfg, sd, "fp64"), R.RefStripedHyena(cfg, sd, "bf16")
    worst_oracle = worst_floor = 0.0
    for p in PROMPTS:
        ids = prepare_batch([p], tok, prepend_bos=False, device="cpu")[0]
        P = ids.shape[1]
        full = torch.cat([ids, reference[p][0][None, :].cpu()], dim=1)
        ref = oracle(full)[0][0][P - 1: P - 1 + N_TOK]
        flo = oracle_bf16(full)[0][0][P - 1: P - 1 + N_TOK]
        worst_oracle = max(worst_oracle, rel_l2(reference[p][1], ref))
        worst_floor = max(worst_floor, rel_l2(flo, ref))
    print(f"[batch-invariant pool, 8 slots] recorded logits vs the fp64 oracle: worst rel-L2 {worst_oracle:.3e} (eager-bf16 oracle {worst_floor:.3e})")
    assert worst_oracle < max(1.5 * worst_floor, 4e-3), (worst_oracle, worst_floor)


# ================================================================================================ the pool at 7B width
# tests/test_gpu_pool.py's WIDE4: D = 4096, 32 heads, 4 layers, one attention layer, interpolated rotary / 16; its inner size is padded to
# 11,008, so every dense layer of the step meets the row-invariant launches' contract -- and takes the routes the toy model never reaches:
# the 3-wave wide launch (Wqkv and the projections, 12288 x 4096), the 4-wave split over K at 16 and at 43 units (4096 x 4096, 4096 x 11008),
# the gate at I = 11008.  The slot counts are the row counts at which the DEFAULT step changes form (fused dot2 up to 4 rows, staged
# 5-8, k-split and n-split MFMA from 9, split over K from 17 and 33); 64 slots leave most slots idle.
WIDE_N_TOK = 8
# six prompts of 17 to 176 tokens.  The fp64 oracle's FFT convolution builds a plan per sequence length (about a second each on torch's
# eager GPU kernels, twice per job: fp64 and the bf16 restatement's fp32); prompt + 8 tokens here are the lengths tests/test_gpu_pool.py's
# D = 4096 cases reach with prompt + 24 (25, 32, 93, 103, 169, 184), so one process pays for each plan once
WIDE_LENGTHS = [95, 24, 161, 17, 85, 176]
WIDE_PROMPTS = [_prompt(n, 200 + i) for i, n in enumerate(WIDE_LENGTHS)]
WIDE_LONG = _prompt(1900, 98)                                          # 1,900 + 8 keys of capacity: past the 1,857 from which the default split count is 32


@pytest.fixture(scope="module")
def wide():
    from evo_amd.tokenizer import CharLevelTokenizer
    from test_gpu_pool import PROMPTS as POOL_PROMPTS, WIDE4
    assert [n + WIDE_N_TOK for n in WIDE_LENGTHS] == [len(p) + 24 for p in POOL_PROMPTS] and len(set(WIDE_LENGTHS)) == 6
    cfg, sd, m = build(dict(WIDE4, use_interpolated_rotary_pos_emb=True, rotary_emb_scaling_factor=16))
    assert m.hidden_size == 4096 and m.num_heads == 32
    return cfg, sd, m, CharLevelTokenizer(512)


def _run_wide(wide, n_slots, prompts=WIDE_PROMPTS, **kw):
    kw.setdefault("n_tokens", [WIDE_N_TOK] * len(prompts))
    return _run(wide, n_slots, prompts=prompts, **kw)


@pytest.fixture(scope="module")
def wide_reference(wide):
    return _run_wide(wide, 8)


@pytest.mark.parametrize("n_slots", [1, 4, 5, 9, 17, 33, 64])
def test_wide_any_slot_count(wide, wide_reference, n_slots):
    _same(_run_wide(wide, n_slots), wide_reference, f"D = 4096, {n_slots} slots against 8", prompts=WIDE_PROMPTS)


def test_wide_any_order(wide, wide_reference):
    n = len(WIDE_PROMPTS)
    _same(_run_wide(wide, 3, prompts=WIDE_PROMPTS[::-1], streams=list(range(n))[::-1]), wide_reference, "D = 4096, prompts in reversed order",
          prompts=WIDE_PROMPTS)


def test_wide_any_company_any_capacity(wide, wide_reference):
    n = len(WIDE_PROMPTS)
    got = _run_wide(wide, 4, prompts=WIDE_PROMPTS + [WIDE_LONG])
    assert len(WIDE_LONG) + WIDE_N_TOK > 1857 > max(WIDE_LENGTHS) + WIDE_N_TOK and got[WIDE_LONG][4] == WIDE_N_TOK and n == 6
    _same(got, wide_reference, "D = 4096, beside a 1,900-token prompt", prompts=WIDE_PROMPTS)


def test_wide_paged(wide, wide_reference):
    _same(_run_wide(wide, 3, pool_kw=dict(kv_paged=True, kv_page_tokens=64)), wide_reference, "D = 4096, kv_paged, 64-token pages", prompts=WIDE_PROMPTS)


def test_wide_eager(wide, wide_reference, monkeypatch):
    monkeypatch.setenv("EVO_AMD_DECODE_GRAPH", "0")
    _same(_run_wide(wide, 5, pool_kw=dict(use_graph=False)), wide_reference, "D = 4096, eager launches", prompts=WIDE_PROMPTS)


def test_wide_default_pool_sees_the_slot_count(wide):
    """Teeth: the DEFAULT pool on the same jobs, 1 slot against 9: the recorded logits of at least one job differ -- these jobs can see what
    the option removes."""
    a, b = _run_wide(wide, 1, batch_invariant=False), _run_wide(wide, 9, batch_invariant=False)
    differ = [len(p) for p in WIDE_PROMPTS if not torch.equal(a[p][1][:WIDE_N_TOK], b[p][1][:WIDE_N_TOK])]
    print(f"[batch-invariant pool, D = 4096, teeth] default pool, 1 slot against 9: recorded logits differ for {len(differ)} of {len(WIDE_PROMPTS)} "
          f"jobs (prompt lengths {differ})")
    assert differ, "the default pool is slot-count-invariant on these jobs: they cannot see a summation order"


_WIDE_PAIRS = {}


def _wide_pair(wide, wide_reference, j):
    """(rel-L2 of job j's recorded logits against the fp64 oracle forward on prompt + generated tokens, the eager-bf16 oracle's), once per
    job.  The oracles run on torch's eager GPU kernels (checker only), as in tests/test_gpu_pool.py at D = 4096."""
    from evo_amd.scoring import prepare_batch
    cfg, sd, m, tok = wide
    if "oracles" not in _WIDE_PAIRS:
        osd = {k: v.to(DEV) for k, v in sd.items()}
        _WIDE_PAIRS["oracles"] = (R.RefStripedHyena(cfg, osd, "fp64", device=DEV), R.RefStripedHyena(cfg, osd, "bf16", device=DEV))
    if j not in _WIDE_PAIRS:
        oracle, oracle_bf16 = _WIDE_PAIRS["oracles"]
        p = WIDE_PROMPTS[j]
        ids = prepare_batch([p], tok, prepend_bos=False, device=DEV)[0]
        P = ids.shape[1]
        full = torch.cat([ids, wide_reference[p][0][None, :].to(DEV)], dim=1)
        ref = oracle(full)[0][0][P - 1: P - 1 + WIDE_N_TOK].cpu()
        flo = oracle_bf16(full)[0][0][P - 1: P - 1 + WIDE_N_TOK].cpu()
        _WIDE_PAIRS[j] = (rel_l2(wide_reference[p][1], ref), rel_l2(flo, ref))
    return _WIDE_PAIRS[j]


@pytest.mark.parametrize("j", range(len(WIDE_LENGTHS)))
def test_wide_oracle_forward_of_one_job(wide, wide_reference, j):
    """One job's pair (split by job: a sequence length costs the oracle's FFT a plan of its own).  The rule is applied to the worst of the
    six below; here only that the pair exists and is a pair of small numbers."""
    got, floor = _wide_pair(wide, wide_reference, j)
    print(f"[batch-invariant pool, D = 4096, 8 slots] job {j} ({WIDE_LENGTHS[j]}-token prompt): rel-L2 {got:.3e} (eager-bf16 oracle {floor:.3e})")
    assert 0 < floor < 1 and 0 < got < 1


def test_wide_recorded_logits_against_the_fp64_oracle(wide, wide_reference):
    """tests/PARITY.md row 23's rule exactly as tests/test_gpu_pool.py applies it at D = 4096: worst rel-L2 over the jobs against the fp64
    oracle on the very same tokens below 1.5 x the worst of the oracle's own eager-bf16 restatement, measured in the same run, and never
    below 4e-3."""
    pairs = [_wide_pair(wide, wide_reference, j) for j in range(len(WIDE_PROMPTS))]
    worst_oracle, worst_floor = max(a for a, _ in pairs), max(b for _, b in pairs)
    _WIDE_PAIRS.pop("oracles", None)                                   # (the fp64 weights: 6.5 GB)
    print(f"[batch-invariant pool, D = 4096, 8 slots] recorded logits vs the fp64 oracle: worst rel-L2 {worst_oracle:.3e} "
          f"(eager-bf16 oracle {worst_floor:.3e})")
    assert worst_oracle < max(1.5 * worst_floor, 4e-3), (worst_oracle, worst_floor)
