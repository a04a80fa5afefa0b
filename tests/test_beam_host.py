"""CPU: beam search in the decode pool -- the layers that need no GPU.

  * the written specification (evo_amd/sh/sample.py: beam_select): the seed step, ended beams carried forward, fewer candidates than W,
    NaN and -inf logits, bit-identical logits where the tie order decides, inactive groups and leftover slots untouched;
  * `DecodePool.beam_search` on the toy model with the fp64 oracle backend (tests/beam_ref.BeamOracleOps): the exhaustive case against
    all 16 two-token continuations scored by plain uncached forwards; W = 1 against the greedy pool; W = 2, 3, 4 against a naive beam
    search that re-forwards every hypothesis from scratch (tests/beam_ref.naive_beam_search), with and without stop tokens, with a
    hypothesis that ends early and still wins and groups that end early and are re-filled;
  * every refusal, the optional group, the public function, the script;
  * the two C entries: exported, declared, bound, ABI unchanged, every contract violation refused with -1 before any launch (the
    pointers passed are never dereferenced);
  * resources: both kernels without scratch or spills."""
import csv
import ctypes
import os
import re
from types import SimpleNamespace

import pytest
import torch

import evo_amd
from evo_amd import _build
from evo_amd import constraints as K
from evo_amd import ops as evo_ops
from evo_amd.backend import Backend
from evo_amd.pool import BeamResult, DecodePool, beam_search
from evo_amd.sh import sample as H
from beam_ref import BeamOracleOps, naive_beam_search, toy_model
from test_gpu_pool import PROMPTS
from test_kernel_resources import HIPCC, _metadata
from test_ragged_prefill_host import TOK, RaggedOracleOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG = float("-inf")
A, C, G, T = (ord(c) for c in "ACGT")
TOL = 1e-9
THREE = [PROMPTS[1], PROMPTS[3], PROMPTS[0]]                          # 8, 1 and 81 tokens: the second is shorter than the FIR history (2)
N_TOK = 6


@pytest.fixture(scope="module")
def small():
    return toy_model(BeamOracleOps(torch.float64))


def _pool(m, n_slots, **kw):
    kw.setdefault("allowed_tokens", "ACGT")
    return DecodePool(m, TOK, n_slots=n_slots, device="cpu", share_prompt_kv=True, **kw)


# ------------------------------------------------------------------------------------------------ the specification
def _state(S, cum, ended=(), length=None, ids=None):
    c = torch.full((S,), NEG, dtype=torch.float64)
    for s, v in cum.items():
        c[s] = v
    e = torch.zeros(S, dtype=torch.uint8)
    e[list(ended)] = 1
    return c, e, torch.zeros(S, dtype=torch.int64) if length is None else torch.tensor(length), \
        torch.full((S,), 9, dtype=torch.int64) if ids is None else torch.tensor(ids)


def _rows(S, seed=0):
    return torch.randn(S, 512, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * 3


def test_spec_seed_step_takes_the_w_best_tokens_of_the_one_live_beam():
    x = _rows(4)
    cum, ended, length, ids = _state(4, {0: 0.0})
    p, i, c, e, n = H.beam_select(x, cum, ended, length, ids, 4)
    lp = x[0] - torch.logsumexp(x[0], -1)                             # the specification's association: cum + (x - lse)
    best = torch.sort(lp, descending=True, stable=True)[1][:4]
    assert p.tolist() == [0, 0, 0, 0] and torch.equal(i, best) and torch.equal(c, lp[best]) and n.tolist() == [1] * 4 and not e.any()
    # with a mask and a stop set: only allowed tokens, the stop token ends its beam
    allow, stop = H.allowed_mask(TOK, "ACGT"), H.allowed_mask(TOK, [int(best[0]), G])
    p, i, c, e, n = H.beam_select(x, cum, ended, length, ids, 4, allowed=allow, stop_tokens=stop)
    order = sorted((A, C, G, T), key=lambda v: (-float(lp[v]), v))
    assert i.tolist() == order and e.tolist() == [v == G for v in order] and torch.equal(c, lp[torch.tensor(order)])
    # nothing is changed in place
    assert torch.equal(cum, _state(4, {0: 0.0})[0]) and not ended.any() and (ids == 9).all()


def test_spec_ended_beams_are_carried_and_fewer_candidates_leave_empty_slots():
    x = _rows(3, seed=1)
    allow = H.allowed_mask(TOK, "AC")
    cum, ended, length, ids = _state(3, {0: -1.0, 1: -0.25}, ended=[1], length=[4, 2, 7], ids=[A, 300, 11])
    p, i, c, e, n = H.beam_select(x, cum, ended, length, ids, 3, allowed=allow)
    lp = x[0] - torch.logsumexp(x[0], -1)                             # the specification's association: cum + (x - lse)
    live = sorted([(-(-1.0 + float(lp[v])), 0, v) for v in (A, C)])
    want = sorted([(0.25, 1, 300)] + live)                            # the ended beam offers itself with its own score
    assert [(q, v) for _, q, v in want] == list(zip(p.tolist(), i.tolist()))
    k = [q for _, q, _ in want].index(1)
    assert float(c[k]) == -0.25 and int(n[k]) == 2 and bool(e[k]) and int(i[k]) == 300      # score, length, ids unchanged; still ended
    assert [int(n[j]) for j in range(3) if j != k] == [5, 5]
    # two candidates for three slots: the last slot becomes empty -- parent = s, cum = -inf, not ended, ids and length as they were
    cum, ended, length, ids = _state(3, {0: -1.0}, ended=[2], length=[4, 2, 7], ids=[A, 300, 11])
    p, i, c, e, n = H.beam_select(x, cum, ended, length, ids, 3, allowed=allow)
    assert p.tolist() == [0, 0, 2] and c[2] == NEG and not e[2] and int(i[2]) == 11 and int(n[2]) == 7
    # every beam empty: every slot stays empty
    cum, ended, length, ids = _state(3, {})
    p, i, c, e, n = H.beam_select(x, cum, ended, length, ids, 3)
    assert p.tolist() == [0, 1, 2] and bool(torch.isinf(c).all()) and (i == 9).all()


def test_spec_nan_and_inf_logits_are_never_candidates():
    x = _rows(2, seed=2)
    x[0, 200] = float("nan")                                          # the row's log-sum-exp is NaN: the beam offers nothing
    x[1, C] = NEG
    cum, ended, length, ids = _state(2, {0: -0.5, 1: -3.0})
    p, i, c, e, n = H.beam_select(x, cum, ended, length, ids, 2, allowed=H.allowed_mask(TOK, "AC"))
    assert p.tolist() == [1, 1] and i.tolist() == [A, 9] and c[1] == NEG and not torch.isnan(c).any()
    x = _rows(2, seed=2)
    x[0, 7] = float("inf")                                            # lse = +inf: finite - inf = -inf, inf - inf = NaN
    p, i, c, e, n = H.beam_select(x, cum, ended, length, ids, 2)
    assert p.tolist() == [1, 1] and not torch.isnan(c).any() and not torch.isinf(c).any()


def test_spec_tie_order_is_parent_then_token():
    row = _rows(1, seed=3)[0]
    row[A] = row[C] = row[T] = 12.0                                   # bit-identical logits in one row
    x = row[None].repeat(5, 1)
    cum, ended, length, ids = _state(5, {0: -1.0, 1: -1.0, 2: -1.0, 3: -1.0})
    p, i, c, e, n = H.beam_select(x, cum, ended, length, ids, 4)
    assert p.tolist() == [0, 0, 0, 1, 4] and i.tolist()[:4] == [A, C, T, A] and len(set(c[:4].tolist())) == 1
    cum[1] = -0.0
    cum[0] = 0.0                                                      # -0 and +0 are one value: the parent decides
    p, i, c, e, n = H.beam_select(x, cum, ended, length, ids, 4)
    assert p.tolist()[:4] == [0, 0, 0, 1]


def test_spec_leaves_inactive_groups_and_leftover_slots_alone():
    x = _rows(7, seed=4)
    cum, ended, length, ids = _state(7, {0: -1.0, 2: -2.0, 3: -0.5, 4: -1.0, 6: -3.0}, ended=[3], length=list(range(7)), ids=list(range(20, 27)))
    p, i, c, e, n = H.beam_select(x, cum, ended, length, ids, 2, group_active=torch.tensor([1, 0, 1]))
    assert p[2:4].tolist() == [2, 3] and p[6] == 6
    for got, was in ((i, ids), (c, cum), (e, ended.bool()), (n, length)):
        assert torch.equal(got[2:4], was[2:4]) and got[6] == was[6]
    assert p[:2].tolist() == [0, 0] and p[4:6].tolist() == [4, 4] and n[:2].tolist() == [1, 1] and n[4:6].tolist() == [5, 5]
    for bad in (0, 9):
        with pytest.raises(ValueError):
            H.beam_select(x, cum, ended, length, ids, bad)
    with pytest.raises(ValueError):
        H.beam_select(x[:3], cum[:3], ended[:3], length[:3], ids[:3], 4)


# ------------------------------------------------------------------------------------------------ the pool against plain forwards
def _full_score(m, prompt, toks):
    """Sum of log-probabilities of `toks` after `prompt`: ONE uncached forward of the full sequence, fp64."""
    ids = list(prompt.encode()) + list(toks)
    with torch.inference_mode():
        lp = torch.log_softmax(m(torch.tensor([ids]))[0][0].double(), -1)
    P = len(prompt)
    return float(sum(lp[P - 1 + k, t] for k, t in enumerate(toks)))


def test_exhaustive_two_tokens_the_best_eight_of_sixteen(small):
    for prompt in (PROMPTS[1], PROMPTS[3]):
        res = _pool(small, 8).beam_search([prompt], n_tokens=2, beam_width=8)[0]
        every = sorted(((-_full_score(small, prompt, (a, b)), (a, b)) for a in (A, C, G, T) for b in (A, C, G, T)))
        assert len(every) == 16 and len(res) == 8 and res.lengths == [2] * 8
        assert res.sequences == ["".join(map(chr, t)) for _, t in every[:8]]              # the true best 8, in order
        assert max(abs(s + w) for s, (w, _) in zip(res.scores, every[:8])) <= TOL
        assert res.mean_scores == [s / 2 for s in res.scores]


def test_width_one_is_the_greedy_run(small):
    pool = _pool(small, 3)
    res = pool.beam_search(PROMPTS, n_tokens=N_TOK, beam_width=1)
    greedy = DecodePool(small, TOK, n_slots=3, top_k=1, device="cpu", share_prompt_kv=True, allowed_tokens="ACGT")
    seqs, _, _ = greedy.generate(PROMPTS, n_tokens=N_TOK)
    assert [list(r.sequences[0].encode()) for r in res] == greedy.last_ids.tolist() and [r.sequences[0] for r in res] == seqs
    assert pool.stats["beam_rows_moved"] == 0 and small.ops.beam_calls["select"] > 0


_NAIVE = {}


def naive(m, W, stop):
    if (W, stop) not in _NAIVE:
        _NAIVE[(W, stop)] = [naive_beam_search(m, p, N_TOK, W, "ACGT", stop) for p in THREE]
    return _NAIVE[(W, stop)]


@pytest.mark.parametrize("stop", ["", "A", "G", "ACGT"])
@pytest.mark.parametrize("W,n_slots", [(2, 4), (3, 7), (4, 4)])
def test_pool_equals_the_naive_search(small, W, n_slots, stop):
    """(4, 4): one group for three prompts, every group is re-filled; (3, 7): two groups and a leftover slot."""
    pool = _pool(small, n_slots, poll_every=3)
    res = pool.beam_search(THREE, n_tokens=N_TOK, beam_width=W, stop_tokens=stop or None)
    want = naive(small, W, stop)
    for r, hyps in zip(res, want):
        assert r.sequences == ["".join(map(chr, t[:-1] if e else t)) for t, _, e in hyps]
        assert r.lengths == [len(t) for t, _, _ in hyps] and max(abs(a - s) for a, (_, s, _) in zip(r.scores, hyps)) <= TOL
        assert r.scores == sorted(r.scores, reverse=True)
    assert pool.stats["beam_groups"] == 3 and pool.stats["prompt_kv_installs"] == 3 and pool.store_refs == [0] * len(pool.store_refs)
    assert not bool(pool._beam["active"].any()) and pool.stats["beam_steps"] == pool.stats["steps"]
    if stop == "A":
        # prompt 0: a hypothesis that ends on its first token (empty string, length 1) and still wins
        assert res[0].sequences[0] == "" and res[0].lengths[0] == 1 and res[0].lengths[1] == N_TOK
    if stop == "ACGT":
        # every hypothesis ends on its first token: each group is over after its admission, fetched and re-filled; no step ever runs
        assert all(r.lengths == [1] * min(W, 4) and r.sequences == [""] * min(W, 4) for r in res) and pool.stats["beam_steps"] == 0
    if stop == "":
        assert pool.stats["polls"] == 0 and pool.stats["beam_rows_moved"] > 0            # without a stop rule nothing is read


def test_a_group_that_ends_early_is_fetched_and_refilled_while_the_other_goes_on(small):
    """Stop token G at W = 2: prompt 1 (a single C) has both hypotheses ended after two steps, the others run to the limit.  With two
    groups for three prompts the early group takes prompt 2 while prompt 0 is still searching; the results do not care."""
    stop = "CG"
    want = [naive_beam_search(small, p, N_TOK, 2, "ACGT", stop) for p in THREE]
    ended_early = [all(e for _, _, e in h) and max(len(t) for t, _, _ in h) < N_TOK for h in want]
    assert any(ended_early) and not all(ended_early), want
    runs = {}
    for poll in (1, 8):
        pool = _pool(small, 4, poll_every=poll)
        res = pool.beam_search(THREE, n_tokens=N_TOK, beam_width=2, stop_tokens=stop)
        for r, hyps in zip(res, want):
            assert r.sequences == ["".join(map(chr, t[:-1] if e else t)) for t, _, e in hyps]
            assert max(abs(a - s) for a, (_, s, _) in zip(r.scores, hyps)) <= TOL
        runs[poll] = pool.stats
    print({k: (v["polls"], v["beam_steps"]) for k, v in runs.items()})
    assert runs[1]["polls"] >= runs[8]["polls"] > 0 and runs[1]["beam_steps"] <= runs[8]["beam_steps"]
    assert runs[1]["beam_steps"] < 2 * (N_TOK - 1)                     # fewer steps than two full rounds of groups


def test_return_steps_prefill_batch_and_the_public_function(small):
    pool = _pool(small, 4, prefill_batch=4)
    res = pool.beam_search(THREE, n_tokens=N_TOK, beam_width=2, return_steps=True)
    one = _pool(small, 4).beam_search(THREE, n_tokens=N_TOK, beam_width=2)
    for r, q in zip(res, one):
        # (sequences, ranks and lengths: exact.  The scores are not compared: the batched prefill hands over end states that differ from the
        # B = 1 prefill's at the 1e-7 level on this backend -- tests/test_ragged_prefill_host.py's subject, not a beam-search quantity)
        assert r.sequences == q.sequences and r.lengths == q.lengths and r.scores == sorted(r.scores, reverse=True) and q.steps is None
        hp, hi, hc = r.steps
        assert tuple(hp.shape) == tuple(hi.shape) == tuple(hc.shape) == (2, N_TOK)
        assert [float(v) for v in hc[:, -1]] == r.scores and [chr(int(v)) for v in hi[:, -1]] == [s[-1] for s in r.sequences]
    assert pool.stats["prefills"] < 3 and pool.stats["prefill_prompts"] == 3             # prompts admitted together share a forward
    # evo_amd.beam_search is DecodePool.beam_search on a pool of its own
    pub = evo_amd.beam_search(THREE, small, TOK, n_tokens=N_TOK, beam_width=2, allowed_tokens="ACGT", device="cpu")
    assert evo_amd.beam_search is beam_search and evo_amd.BeamResult is BeamResult
    assert [(r.sequences, r.scores, r.lengths) for r in pub] == [(r.sequences, r.scores, r.lengths) for r in one]
    assert isinstance(pub[0], BeamResult) and len(pub[0]) == 2
    # a second search on the same pool reuses its state; a wider one makes new state
    state = pool._beam
    again = pool.beam_search(THREE[:2], n_tokens=3, beam_width=2, stop_tokens="G")
    fresh = _pool(small, 4, prefill_batch=4).beam_search(THREE[:2], n_tokens=3, beam_width=2, stop_tokens="G")
    assert pool._beam is not state                                    # (a stop set is part of the state's key: new state on the same caches)
    state = pool._beam
    third = pool.beam_search(THREE[1:], n_tokens=3, beam_width=2, stop_tokens="A")
    assert pool._beam is state                                        # the same width, history and caches: the state is reused
    fresh3 = _pool(small, 4, prefill_batch=4).beam_search(THREE[1:], n_tokens=3, beam_width=2, stop_tokens="A")
    for got, want in ((again, fresh), (third, fresh3)):
        assert [(r.sequences, r.scores, r.lengths) for r in got] == [(r.sequences, r.scores, r.lengths) for r in want]     # a fresh pool's, to the bit
    assert len(pool.beam_search(THREE[:1], n_tokens=3, beam_width=4)[0]) == 4


# ------------------------------------------------------------------------------------------------ what is refused
def test_what_is_refused(small, monkeypatch):
    calls = []
    embed = small.ops.embed
    monkeypatch.setattr(small.ops, "embed", lambda *a, **kw: (calls.append(1), embed(*a, **kw))[1])
    pool = _pool(small, 4)
    for bad in (0, 9, -1, 5):                                         # outside 1 ... 8, or larger than n_slots
        with pytest.raises(ValueError, match="beam_width"):
            pool.beam_search(THREE, n_tokens=3, beam_width=bad)
    with pytest.raises(ValueError, match="share_prompt_kv"):
        DecodePool(small, TOK, n_slots=4, device="cpu").beam_search(THREE, n_tokens=3)
    with pytest.raises(ValueError):                                   # such pools are refused where they are built
        DecodePool(small, TOK, n_slots=4, device="cpu", share_prompt_kv=True, kv_dtype="fp8")
    with pytest.raises(ValueError):
        DecodePool(small, TOK, n_slots=4, device="cpu", share_prompt_kv=True, kv_paged=True)
    for kw in (dict(constraints=K.iupac_template("ACGT")), dict(stop_sequences=["TAA"]), dict(seed=3)):
        with pytest.raises(ValueError, match=next(iter(kw))):
            pool.beam_search(THREE, n_tokens=3, **kw)
    with pytest.raises(TypeError):
        pool.beam_search(THREE, n_tokens=3, top_k=4)
    for n in (0, -2):
        with pytest.raises(ValueError, match="n_tokens"):
            pool.beam_search(THREE, n_tokens=n)
    with pytest.raises(ValueError, match="empty"):
        pool.beam_search([], n_tokens=3)
    with pytest.raises(ValueError, match="prompt"):
        pool.beam_search(["ACGT", ""], n_tokens=3)
    with pytest.raises(ValueError):
        beam_search(THREE, small, TOK, n_tokens=3, beam_width=9)
    with pytest.raises(ValueError):
        beam_search([], small, TOK, n_tokens=3)
    assert calls == [] and pool.ipd is None                           # every refusal came before any device work
    # a backend without the group
    assert Backend.OPTIONAL["beam"] == ("beam_select", "gather_rows")
    plain = toy_model(RaggedOracleOps(torch.float64))
    assert small.ops.supports("beam") and not plain.ops.supports("beam")
    with pytest.raises(RuntimeError, match="beam"):
        DecodePool(plain, TOK, n_slots=4, device="cpu", share_prompt_kv=True, allowed_tokens="ACGT").beam_search(THREE, n_tokens=3)
    for meth in Backend.OPTIONAL["beam"] + ("gather_table",):
        assert hasattr(evo_ops.HipOps, meth), meth


def test_default_slot_count_of_the_public_function(small, monkeypatch):
    seen = []

    class RecordingPool:
        def __init__(self, model, tok, **kw):
            seen.append(kw)

        def beam_search(self, prompts, n_tokens, **kw):
            seen.append(kw)
            return []
    monkeypatch.setattr(evo_amd.pool, "DecodePool", RecordingPool)
    for n_prompts, W, want in ((3, 4, 12), (40, 4, 32), (40, 3, 30), (1, 8, 8), (9, 5, 30)):
        evo_amd.pool.beam_search(["A"] * n_prompts, None, None, n_tokens=2, beam_width=W)
        assert seen[-2]["n_slots"] == want and seen[-2]["share_prompt_kv"] is True and seen[-1]["beam_width"] == W


# ------------------------------------------------------------------------------------------------ the script
def test_the_script_writes_one_row_per_hypothesis(small, tmp_path, monkeypatch):
    import scripts.beam_search as cli
    monkeypatch.setattr(evo_amd, "Evo", lambda *a, **kw: SimpleNamespace(model=small, tokenizer=TOK))
    (tmp_path / "p.fa").write_text(">a\n" + THREE[0] + "\n>b\n" + THREE[1] + "\n")
    out = tmp_path / "out.csv"
    rows = cli.main(["--prompts", str(tmp_path / "p.fa"), "--output-csv", str(out), "--beam-width", "3", "--n-tokens", "4",
                     "--allowed-tokens", "ACGT", "--stop-tokens", "G", "--device", "cpu"])
    want = _pool(small, 6).beam_search(THREE[:2], n_tokens=4, beam_width=3, stop_tokens="G")
    got = list(csv.reader(open(out)))
    assert got[0] == ["Prompt Id", "Rank", "Sequence", "Score", "Length"] and got[1:] == rows and len(rows) == 6
    for pi, r in enumerate(want):
        mine = [g for g in got[1:] if g[0] == str(pi)]
        assert [g[1] for g in mine] == ["0", "1", "2"] and [g[2] for g in mine] == r.sequences
        assert [float(g[3]) for g in mine] == r.scores and [int(g[4]) for g in mine] == r.lengths
    # the documented invocation: a stop token outside the allowed set can never be chosen and changes nothing
    doc = cli.main(["--prompts", str(tmp_path / "p.fa"), "--output-csv", str(out), "--beam-width", "4", "--n-tokens", "5",
                    "--allowed-tokens", "ACGT", "--stop-tokens", "N", "--device", "cpu"])
    plain = _pool(small, 8).beam_search(THREE[:2], n_tokens=5, beam_width=4)
    assert [r[2] for r in doc] == [q for r in plain for q in r.sequences] and [float(r[3]) for r in doc] == [q for r in plain for q in r.scores]
    assert all(r[4] == "5" for r in doc) and len(doc) == 8
    for bad in (["--beam-width", "9"], ["--n-tokens", "0"], ["--beam-width", "4", "--n-slots", "3"]):
        with pytest.raises(SystemExit):
            cli.main(["--prompts", str(tmp_path / "p.fa"), "--output-csv", str(out)] + bad)


# ------------------------------------------------------------------------------------------------ C ABI
ENTRIES = ("evo_beam_select_f32", "evo_gather_rows")
ONE = ctypes.c_void_p(16)                                             # non-null, 16-byte aligned, never dereferenced


def _caller(name, names, ok):
    f = getattr(evo_ops.load_library(), name)
    assert list(ok) == names and len(evo_ops._SIGNATURES[name][0]) == len(names)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return f(*[a[n] for n in names])
    return call


def test_entries_are_wired():
    header = open(os.path.join(ROOT, "include", "evo_mi355x.h")).read()
    for name in ENTRIES:
        assert name in _build.EXPORTS and name in evo_ops._SIGNATURES and re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert int(re.search(r"#define EVO_ABI_VERSION (\d+)", header).group(1)) == evo_ops.ABI_VERSION == 20      # additive: no signature changed
    assert evo_ops.load_library().evo_abi_version() == 20
    assert any(p.name == "beam.hip" for p in _build.sources())
    import inspect
    assert {"beam_width", "stop_tokens", "prepend_bos", "return_steps"} <= set(inspect.signature(DecodePool.beam_search).parameters)
    assert {"beam_width", "n_slots", "allowed_tokens", "stop_tokens", "prefill_batch", "weight_dtype", "device"} \
        <= set(inspect.signature(beam_search).parameters)


def test_beam_select_refuses_before_any_launch():
    names = ["logits", "logits_f32", "ld", "allow", "stop_mask", "group_active", "cum", "ended", "length", "ids", "parent", "hist_parent",
             "hist_ids", "hist_cum", "hist_len", "step", "t", "W", "S", "V", "stream"]
    ok = dict(logits=ONE, logits_f32=0, ld=512, allow=None, stop_mask=None, group_active=None, cum=ONE, ended=ONE, length=ONE, ids=ONE,
              parent=ONE, hist_parent=ONE, hist_ids=ONE, hist_cum=None, hist_len=4, step=None, t=0, W=4, S=9, V=512, stream=None)
    call = _caller("evo_beam_select_f32", names, ok)
    for n in ("logits", "cum", "ended", "length", "ids", "parent"):
        assert call(**{n: None}) == -1, n
    assert call(logits=ctypes.c_void_p(8)) == -1 and call(cum=ctypes.c_void_p(18)) == -1
    for n in ("length", "ids", "parent", "hist_ids"):
        assert call(**{n: ctypes.c_void_p(20)}) == -1, n
    assert call(hist_parent=ctypes.c_void_p(18)) == -1 and call(hist_cum=ctypes.c_void_p(18)) == -1 and call(step=ctypes.c_void_p(20)) == -1
    for kw in (dict(W=0), dict(W=9), dict(W=-1), dict(S=3), dict(S=0), dict(S=1 << 31), dict(V=256), dict(ld=504), dict(ld=516)):
        assert call(**kw) == -1, kw
    # a step to record -- t >= 0, or the device step vector -- without its history
    for kw in (dict(hist_parent=None), dict(hist_ids=None), dict(hist_len=0), dict(t=-1, step=ONE, hist_parent=None),
               dict(t=-1, step=ONE, hist_len=0)):
        assert call(**kw) == -1, kw


def test_gather_rows_refuses_before_any_launch():
    names = ["table", "n_entries", "parent", "own_pos", "scratch", "scratch_row_bytes", "max_row_bytes", "S", "back", "stream"]
    ok = dict(table=ONE, n_entries=3, parent=ONE, own_pos=ONE, scratch=ONE, scratch_row_bytes=4096, max_row_bytes=1024, S=8, back=0,
              stream=None)
    call = _caller("evo_gather_rows", names, ok)
    for n in ("table", "parent", "own_pos", "scratch"):
        assert call(**{n: None}) == -1, n
    for n in ("table", "parent", "own_pos"):
        assert call(**{n: ctypes.c_void_p(20)}) == -1, n
    assert call(scratch=ctypes.c_void_p(24)) == -1
    for kw in (dict(n_entries=0), dict(n_entries=65536), dict(S=0), dict(S=65536), dict(scratch_row_bytes=0), dict(scratch_row_bytes=4104),
               dict(max_row_bytes=0), dict(max_row_bytes=1032), dict(max_row_bytes=8192), dict(back=2), dict(back=-1)):
        assert call(**kw) == -1, kw


# ------------------------------------------------------------------------------------------------ resources
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_beam_kernels_need_no_scratch():
    meta = _metadata("beam.hip")
    kernels = {k: r for k, r in meta.items() if any(n in k for n in ("beam_select_kernel", "gather_rows_kernel"))}
    assert len(kernels) == 2 == len(meta), sorted(meta)
    print(f"[beam] {kernels}")
    for name, r in kernels.items():
        assert r["scratch"] == 0 and r["spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
    sel = next(r for k, r in kernels.items() if "beam_select_kernel" in k)
    cp = next(r for k, r in kernels.items() if "gather_rows_kernel" in k)
    # the selection: 8 waves of one workgroup on one CU -- at most 64 registers each and far less LDS than the sampler's sort (6,144 bytes)
    assert sel["vgpr"] <= 64 and sel["lds"] <= 1024, sel
    assert cp["vgpr"] <= 32 and cp["lds"] == 0, cp                    # a copy: nothing but addresses and the vectors in flight
    sampler = _metadata("sample.hip")
    assert all(r["scratch"] == 0 and r["spill"] == 0 for r in sampler.values()) and len(sampler) == 3      # the shared header cost them nothing
