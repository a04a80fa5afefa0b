"""GPU (-m gpu): seeded, restricted sampling in the decode pool and in `generate` -- the device sampler as the last node of the
pooled step (evo_amd/pool.py, csrc/sample.hip).  Same seed and slot count: same ids, logits and scores; the recorded logits are
still the engine's parallel forward on (prompt + generated tokens), by the rule of tests/test_gpu_pool.py; and every generated
token is the one the written specification (sh/sample.py sample_seeded) draws from the recorded logits row with the job's
(seed, stream = output index, count = position) -- which pins the pool's wiring of the random streams."""
import numpy as np
import pytest
import torch

from test_gpu_model import DEV, SMALL4, build
from test_gpu_pool import PROMPTS, WIDE4
from test_gpu_sample import accept

pytestmark = pytest.mark.gpu
N_TOK = 24


def make(dims):
    from evo_amd.tokenizer import CharLevelTokenizer
    cfgd = dict(SMALL4 if dims == "toy" else WIDE4, use_interpolated_rotary_pos_emb=True, rotary_emb_scaling_factor=16)
    return build(cfgd)[2], CharLevelTokenizer(512)


def run(m, tok, n_slots, use_graph, seed, prompts=PROMPTS, **kw):
    from evo_amd.pool import DecodePool
    gen = {k: kw.pop(k) for k in ("sampling", "streams") if k in kw}
    pool = DecodePool(m, tok, n_slots=n_slots, top_k=kw.pop("top_k", 4), top_p=kw.pop("top_p", 1.0), temperature=kw.pop("temperature", 0.7),
                      device=DEV, use_graph=use_graph, seed=seed, **kw)
    seqs, scores, owner = pool.generate(prompts, n_tokens=N_TOK, n_sample_per_prompt=2, **gen)
    return pool, seqs, scores, owner


def accepted(pool, seed, top_k, top_p, temperature, mask=None, streams=None):
    """(share of rows left out, number of tokens the specification rejects) over every generated token of a finished job."""
    n_jobs = pool.last_ids.shape[0]
    rows = pool.last_logits.reshape(n_jobs * N_TOK, 512)
    st = np.repeat(np.arange(n_jobs) if streams is None else np.asarray(streams), N_TOK)
    ct = np.tile(np.arange(N_TOK), n_jobs)
    out, bad = accept(rows, pool.last_ids.reshape(-1), top_k, top_p, temperature, mask, seed, st, ct)
    return out.float().mean().item(), int(bad.sum())


@pytest.mark.parametrize("dims,n_slots,use_graph", [("toy", 4, True), ("toy", 3, False), ("d4096", 8, True)])
def test_same_seed_same_samples_and_the_streams_are_wired(dims, n_slots, use_graph):
    from evo_amd.scoring import prepare_batch
    m, tok = make(dims)
    a, seqs_a, scores_a, owner = run(m, tok, n_slots, use_graph, seed=5)
    b, seqs_b, scores_b, _ = run(m, tok, n_slots, use_graph, seed=5)
    assert owner == [i for i in range(len(PROMPTS)) for _ in range(2)] and a.stats["prefills"] == len(PROMPTS)
    assert a.stats["tokens"] == len(seqs_a) * (N_TOK - 1)
    assert torch.equal(a.last_ids, b.last_ids) and torch.equal(a.last_logits, b.last_logits)
    assert seqs_a == seqs_b and scores_a == scores_b
    assert all(s == s and s <= 0 for s in scores_a)
    c, seqs_c, _, _ = run(m, tok, n_slots, use_graph, seed=6)
    assert not torch.equal(a.last_ids, c.last_ids)
    assert (a.last_ids[0::2] != a.last_ids[1::2]).any()                # the two samples of a prompt are different streams
    # the recorded logits are the parallel forward's (rule and tolerance of tests/test_gpu_pool.py)
    worst = 0.0
    for j, pi in enumerate(owner):
        ids = prepare_batch([PROMPTS[pi]], tok, prepend_bos=False, device=DEV)[0]
        P = ids.shape[1]
        full_ids = torch.cat([ids, a.last_ids[j: j + 1].to(DEV)], dim=1)
        with torch.inference_mode():
            full = m(full_ids)[0][0].float().cpu()
        want = full[P - 1: P - 1 + N_TOK]
        worst = max(worst, ((a.last_logits[j] - want).norm() / want.norm()).item())
    share, bad = accepted(a, 5, 4, 1.0, 0.7)
    print(f"[seeded pool {dims} {n_slots} slots, graph={use_graph}] recorded logits vs the parallel forward: worst rel-L2 {worst:.3e}; "
          f"tokens rejected by sample_seeded {bad}, rows left out {100 * share:.2f} %")
    assert worst < 2e-2, worst
    assert share <= 0.04 and bad == 0, (share, bad)


def test_allowed_tokens_and_per_prompt_settings():
    from evo_amd.sh.sample import allowed_mask
    m, tok = make("toy")
    # top-p sampling over everything the mask leaves
    pool, seqs, scores, owner = run(m, tok, 4, True, seed=3, top_k=0, top_p=0.9, temperature=1.0, allowed_tokens="ACGT")
    assert all(len(s) == N_TOK and set(s) <= set("ACGT") for s in seqs), seqs
    mask = allowed_mask(tok, "ACGT")
    share, bad = accepted(pool, 3, 0, 0.9, 1.0, mask)
    print(f"[seeded pool, ACGT only] tokens rejected {bad}, rows left out {100 * share:.2f} %")
    assert share <= 0.04 and bad == 0
    # without a seed the mask alone still moves the sampler onto the device (seed 0)
    pool0, seqs0, _, _ = run(m, tok, 4, True, seed=None, allowed_tokens="ACGT")
    assert pool0.device_sampler and all(set(s) <= set("ACGT") for s in seqs0)
    # per-prompt settings: greedy for prompt 0, the pool's own for the rest
    sampling = [dict(top_k=1)] + [None] * (len(PROMPTS) - 1)
    pool, seqs, _, owner = run(m, tok, 4, True, seed=3, sampling=sampling)
    assert torch.equal(pool.last_ids[0], pool.last_logits[0].argmax(-1)) and torch.equal(pool.last_ids[0], pool.last_ids[1])
    share, bad = accepted_subset(pool, 3, 2)
    assert bad == 0


def accepted_subset(pool, seed, first_job):
    n_jobs = pool.last_ids.shape[0]
    rows = pool.last_logits[first_job:].reshape(-1, 512)
    st = np.repeat(np.arange(first_job, n_jobs), N_TOK)
    ct = np.tile(np.arange(N_TOK), n_jobs - first_job)
    out, bad = accept(rows, pool.last_ids[first_job:].reshape(-1), 4, 1.0, 0.7, None, seed, st, ct)
    return out.float().mean().item(), int(bad.sum())


def test_reversed_prompt_order_with_the_streams_carried():
    """The same prompts in reversed order, same slot count and seed, every output keeping its random stream: each token is the
    specification's draw from its own recorded logits, and the samples are IDENTICAL -- which rests on a row's logits not depending on
    the slot it sits in or on its neighbours' positions (for one slot count); measured to hold bit for bit."""
    m, tok = make("toy")
    a, seqs_a, _, _ = run(m, tok, 4, True, seed=9)
    n = len(PROMPTS)
    streams = [2 * (n - 1 - pi) + c for pi in range(n) for c in range(2)]
    b, seqs_b, _, _ = run(m, tok, 4, True, seed=9, prompts=PROMPTS[::-1], streams=streams)
    share, bad = accepted(b, 9, 4, 1.0, 0.7, streams=streams)
    assert share <= 0.04 and bad == 0, (share, bad)
    back = [seqs_b[streams.index(j)] for j in range(2 * n)]
    same = sum(x == y for x, y in zip(seqs_a, back))
    lg_b = torch.stack([b.last_logits[streams.index(j)] for j in range(2 * n)])
    print(f"[seeded pool, reversed prompt order] identical samples: {same} of {2 * n}; recorded logits bit-identical: "
          f"{bool(torch.equal(a.last_logits, lg_b))}; first tokens identical: {bool(torch.equal(a.last_ids[:, 0], torch.stack([b.last_ids[streams.index(j)] for j in range(2 * n)])[:, 0]))}")
    # measured on the MI355X: a row's logits do not depend on its slot or on its neighbours -- bit-identical logits, identical samples
    assert same == 2 * n and torch.equal(a.last_logits, lg_b)


def test_generate_with_a_seed_repeats_and_the_default_path_is_untouched(monkeypatch):
    import evo_amd
    from evo_amd.ops import HipOps
    m, tok = make("toy")
    calls = []
    real = HipOps.sample_rows

    def counting(self, *a, **kw):
        calls.append(1)
        return real(self, *a, **kw)
    monkeypatch.setattr(HipOps, "sample_rows", counting)
    prompts = ["ACGTACGTAGCTAGCT", "GGATTACAGGATTACA", "TTTTACGATTACAGAT"]
    kw = dict(n_tokens=12, temperature=0.7, top_k=4, top_p=1.0, cached_generation=True, verbose=0, device=DEV)
    s1, sc1 = evo_amd.generate(prompts, m, tok, seed=7, **kw)
    n_calls = len(calls)
    s2, sc2 = evo_amd.generate(prompts, m, tok, seed=7, **kw)
    assert n_calls == 12 and s1 == s2 and all(len(s) == 12 for s in s1) and [float(x) for x in sc1] == [float(x) for x in sc2]
    s3, _ = evo_amd.generate(prompts, m, tok, seed=8, **kw)
    assert s3 != s1
    s4, _ = evo_amd.generate(prompts, m, tok, seed=7, allowed_tokens="ACGT", **kw)
    assert all(set(s) <= set("ACGT") for s in s4)
    # one prompt at a time: consecutive batches of a call use consecutive streams, so equal prompts give different samples
    s5, _ = evo_amd.generate([prompts[0]] * 3, m, tok, seed=7, batched=False, **kw)
    assert len(set(s5)) > 1
    # the wiring of `Generator`: row b of the batch is stream b, token j is draw j
    from evo_amd.generation import Generator
    from evo_amd.scoring import prepare_batch
    ids = prepare_batch(prompts, tok, prepend_bos=False, device=DEV)[0]
    out, logits, _ = Generator(m, tok, top_k=4, top_p=1.0, temperature=0.7, seed=7).generate(
        device=DEV, input_ids=ids, num_tokens=12, cached_generation=True, print_generation=False, stop_at_eos=False)
    assert list(tok.detokenize_batch(out)) == s1
    left, bad = accept(logits.reshape(-1, 512), out.reshape(-1), 4, 1.0, 0.7, None, 7, np.repeat(np.arange(3), 12), np.tile(np.arange(12), 3))
    assert int(bad.sum()) == 0 and left.float().mean().item() <= 0.04
    before = len(calls)
    torch.manual_seed(0)
    evo_amd.generate(prompts, m, tok, **kw)                           # no seed, no mask: the host sampler of the reference
    assert len(calls) == before
