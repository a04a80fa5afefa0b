"""GPU (-m gpu): the decode pool with ONE stored K/V per prompt (DecodePool share_prompt_kv; evo_attn_decode_prefix_bf16 and
evo_rope_append_decode_at_bf16 inside the pooled, captured step).  Record: DESIGN.md section 16.

Body and rule of tests/test_gpu_pool.test_pool_logits_match_parallel_forward: the tokens are taken as the pool sampled them and the
LOGITS it recorded are checked against the fp64 oracle's forward on (prompt + generated tokens) -- max(1.5 x the eager-bf16 oracle's
own rel-L2, 4e-3) -- and against the engine's parallel forward (2e-2).  Three samples per prompt, 24 tokens: with 8 slots a tile of the
grouped kernel holds copies of two or three prompts, slots are re-filled mid-stream and store rows are reused.  The seeded cases are
those of tests/test_gpu_pool_seeded.py on the shared path."""
import pytest
import torch

from oracle import stripedhyena_ref as R
from test_gpu_model import DEV, SMALL4, build, rel_l2
from test_gpu_pool import PROMPTS, WIDE4
from test_gpu_pool_seeded import N_TOK, accepted, make

pytestmark = pytest.mark.gpu
N_SAMPLE = 3


def _stats_ok(pool, n_slots):
    R_ = min(n_slots, -(-n_slots // N_SAMPLE) + 1)
    assert pool.stats["prefills"] == pool.stats["prompt_kv_installs"] == len(PROMPTS)
    assert pool.stats["store_rows"] == R_ and pool.store_refs == [0] * R_
    assert pool.stats["steps"] <= pool.stats["prefix_streams"] <= pool.stats["tokens"]
    for kv in pool.ipd["mha"].key_value_memory_dict.values():
        assert tuple(kv.shape[:2]) == (n_slots, N_TOK)
    for kv in pool.store.kv.values():
        assert tuple(kv.shape[:2]) == (R_, max(len(p) for p in PROMPTS))


@pytest.mark.parametrize("dims,n_slots,use_graph", [("toy", 8, True), ("toy", 3, False), ("d4096", 8, True)])
def test_shared_pool_logits_match_parallel_forward(dims, n_slots, use_graph):
    from evo_amd.pool import DecodePool
    from evo_amd.scoring import prepare_batch
    from evo_amd.tokenizer import CharLevelTokenizer
    tok = CharLevelTokenizer(512)
    cfgd = dict(SMALL4 if dims == "toy" else WIDE4, use_interpolated_rotary_pos_emb=True, rotary_emb_scaling_factor=16)
    cfg, sd, m = build(cfgd)
    odev = None if dims == "toy" else DEV                       # (the wide oracles run on torch's eager GPU kernels: checker only)
    osd = sd if odev is None else {k: v.to(DEV) for k, v in sd.items()}
    oracle, oracle_bf16 = R.RefStripedHyena(cfg, osd, "fp64", device=odev), R.RefStripedHyena(cfg, osd, "bf16", device=odev)
    pool = DecodePool(m, tok, n_slots=n_slots, top_k=4, top_p=1.0, temperature=0.7, device=DEV, use_graph=use_graph, share_prompt_kv=True)
    torch.manual_seed(0)
    seqs, scores, owner = pool.generate(PROMPTS, n_tokens=N_TOK, n_sample_per_prompt=N_SAMPLE)
    assert len(seqs) == N_SAMPLE * len(PROMPTS) and owner == [i for i in range(len(PROMPTS)) for _ in range(N_SAMPLE)]
    _stats_ok(pool, n_slots)
    worst = worst_oracle = worst_floor = 0.0
    for j, pi in enumerate(owner):
        ids = prepare_batch([PROMPTS[pi]], tok, prepend_bos=False, device=DEV)[0]
        P = ids.shape[1]
        full_ids = torch.cat([ids, pool.last_ids[j: j + 1].to(DEV)], dim=1)
        with torch.inference_mode():
            full = m(full_ids)[0][0].float().cpu()                # [P + n, V]
        want = full[P - 1: P - 1 + N_TOK]
        got = pool.last_logits[j]
        worst = max(worst, ((got - want).norm() / want.norm()).item())
        oid = full_ids.cpu() if odev is None else full_ids
        ref = oracle(oid)[0][0][P - 1: P - 1 + N_TOK].cpu()                   # fp64 oracle on the very same tokens
        flo = oracle_bf16(oid)[0][0][P - 1: P - 1 + N_TOK].cpu()
        worst_oracle = max(worst_oracle, rel_l2(got, ref))
        worst_floor = max(worst_floor, rel_l2(flo, ref))
    print(f"[shared pool {dims} {n_slots} slots, graph={use_graph}] recorded logits vs the fp64 oracle: worst rel-L2 {worst_oracle:.3e} "
          f"(eager-bf16 oracle {worst_floor:.3e}); vs the engine's parallel forward {worst:.3e}; stats {pool.stats}")
    assert worst_oracle < max(1.5 * worst_floor, 4e-3), (worst_oracle, worst_floor)
    assert worst < 2e-2, worst
    assert all(s == s and s <= 0 for s in scores)


def _run(m, tok, seed, prompts=PROMPTS, streams=None):
    from evo_amd.pool import DecodePool
    pool = DecodePool(m, tok, n_slots=8, top_k=4, top_p=1.0, temperature=0.7, device=DEV, use_graph=True, seed=seed, share_prompt_kv=True)
    seqs, _, _ = pool.generate(prompts, n_tokens=N_TOK, n_sample_per_prompt=N_SAMPLE, streams=streams)
    return pool, seqs


def test_seeded_shared_pool_repeats_and_keeps_samples_under_reordering():
    """Device sampler on the shared path: the same seed gives the same tokens and logits; with the prompts reversed and every output
    keeping its random stream each prompt's samples are unchanged -- a row's logits depend neither on the slot it sits in, nor on the
    store row it reads, nor on which other prompts share its tile."""
    m, tok = make("toy")
    a, seqs_a = _run(m, tok, 9)
    b, seqs_b = _run(m, tok, 9)
    assert torch.equal(a.last_ids, b.last_ids) and torch.equal(a.last_logits, b.last_logits) and seqs_a == seqs_b
    _stats_ok(a, 8)
    share, bad = accepted(a, 9, 4, 1.0, 0.7)
    assert share <= 0.04 and bad == 0, (share, bad)
    n = len(PROMPTS)
    streams = [N_SAMPLE * (n - 1 - pi) + c for pi in range(n) for c in range(N_SAMPLE)]
    c, seqs_c = _run(m, tok, 9, prompts=PROMPTS[::-1], streams=streams)
    share, bad = accepted(c, 9, 4, 1.0, 0.7, streams=streams)
    assert share <= 0.04 and bad == 0, (share, bad)
    back = [seqs_c[streams.index(j)] for j in range(N_SAMPLE * n)]
    same = sum(x == y for x, y in zip(seqs_a, back))
    lg_c = torch.stack([c.last_logits[streams.index(j)] for j in range(N_SAMPLE * n)])
    print(f"[seeded shared pool, reversed prompt order] identical samples: {same} of {N_SAMPLE * n}; recorded logits bit-identical: "
          f"{bool(torch.equal(a.last_logits, lg_c))}")
    assert same == N_SAMPLE * n and torch.equal(a.last_logits, lg_c)
