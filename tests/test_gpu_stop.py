"""GPU (-m gpu): decode-pool jobs that end on their own -- the control kernel `evo_sample_rows_ctl_f32`
(csrc/sample.hip, HipOps.sample_rows_ctl) against the written rule (evo_amd/sh/sample.py: sample_seeded + finish_reason), and the pool
that runs on it.

  * kernel: 12 consecutive launches over histories of 12 cells; the tokens, counters, `active`, `length`, `finish` and the token history
    equal the specification exactly; token, log-probability and recorded logits are bit-identical to `evo_sample_rows_f32` on the same rows
    and counters; canaries around every unwritten cell stand; the eager launches equal the same launches captured in one graph;
  * arena: the entry inside a poisoned arena, with and without the optional histories.  `covers()` registers the entry point at IMPORT
    time: in a whole-suite run this module is what names `evo_sample_rows_ctl_f32` for tests/test_gpu_arena.py's
    test_every_entry_point_is_named_by_a_case; tests/test_gpu_arena.py run on its own does not import this file and would not see the name;
  * pool: a run with stop codons is, job by job, the PREFIX of the fixed-length run with the same seed and slot count that the rule cuts
    out of it -- ids, finish reasons, log-probabilities bit for bit; the combinations with share_prompt_kv and prefill_batch; scores."""
import numpy as np
import pytest
import torch

from evo_amd.sh import sample as H
from test_gpu_arena import _run, covers, gen, poisoned, rnd
from test_gpu_model import DEV, SMALL4, build
from test_gpu_pool import PROMPTS
from test_gpu_sample import accept, acgt_mask, ops

pytestmark = pytest.mark.gpu
A, C, G, T = (ord(c) for c in "ACGT")
L = 12
SEED = 4242
# one stop token; patterns of 1, 3 and 8 tokens (none holds the stop token, so every one of them can end a job)
STOP_TOKENS = [T]
PATTERNS = [[G], [A, A, C], [A, C, A, C, A, C, A, C]]
# rows 0 ... 4 follow a script (their logits put +60 on the scripted token); what each one shows, frame 1 / frame 3:
SCRIPTS = ["ACACACACACAC",     # the 8-token pattern at n = 8 / at n = 12, where it outranks the length limit 12
           "CAACAACAACAA",     # AAC at n = 4 / never in frame (n = 4, 7, 10): the limit 11 ends it
           "GAGAAAAAAAAA",     # the 1-token pattern on the FIRST token (cnt = 0: the longer patterns read nothing) / G at n = 3
           "AATAAAAAAAAA",     # the stop token at n = 3 = its limit: reason 1 outranks reason 3
           "AAAAAAAAAAAA"]     # inactive from the start: nothing of it may change
SCRIPT_LIMITS = [12, 11, 12, 3, 12]
GONE_ROW = 100                                                        # S = 257: a row whose count is past the history


def _scripted(S):
    """[(script, limit)] of rows 0 ... : the five above; with S = 257 also, for every count 0 ... 11, a row that meets the stop token
    there, one whose limit ends it there, and one that meets the 1-token pattern there (a stop only when n = cnt + 1 is in frame)."""
    rows = list(zip(SCRIPTS, SCRIPT_LIMITS))[:S]
    if S > 5:
        for cnt in range(L):
            rows += [("A" * cnt + "T" + "A" * (L - 1 - cnt), 12), ("A" * L, cnt + 1), ("A" * cnt + "G" + "A" * (L - 1 - cnt), 12)]
    return rows


def _initial(S):
    s = torch.arange(S)
    limit = 1 + s % 12
    sc = _scripted(S)
    limit[: len(sc)] = torch.tensor([lim for _, lim in sc])
    active = s % 7 != 6
    active[: len(sc)] = True
    count = torch.zeros(S, dtype=torch.int64)
    if S > 5:
        gone = (s >= len(sc)) & (s % 11 == 10)
        count[gone] = limit[gone]                                    # active with nothing left to draw: ends by length, draws nothing
        count[GONE_ROW], limit[GONE_ROW], active[GONE_ROW] = L, 99, True            # beyond the history: the same
    if S >= 5:
        active[4] = False
    return limit, active, count


def _rows(S, f32, seed):
    """[L launches, S, 512]: random rows; the scripted rows get +60 on their token of that launch."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(L, S, 512, generator=g) * 3.0).bfloat16()
    for s, (script, _) in enumerate(_scripted(S)):
        for t in range(L):
            x[t, s, ord(script[t])] = 60.0
    return x.float() if f32 else x


def _state(S, limit, active, count, logits_hist=True):
    return dict(count=count.clone().to(DEV), active=active.clone().to(DEV), limit=limit.clone().to(DEV),
                length=torch.full((S,), -5, dtype=torch.int64, device=DEV), finish=torch.full((S,), 9, dtype=torch.uint8, device=DEV),
                ids=torch.full((S,), -7, dtype=torch.int64, device=DEV), lp=torch.full((S,), 123.0, dtype=torch.float32, device=DEV),
                hid=torch.full((S, L), -9, dtype=torch.int64, device=DEV), hlp=torch.full((S, L), 777.0, dtype=torch.float32, device=DEV),
                hlg=torch.full((S, L, 512), 777.0, dtype=torch.float32, device=DEV) if logits_hist else None)


def _launch(st, rows, prm, stream, allow, stop_mask, stop_seq, frame):
    ops().sample_rows_ctl(rows, *prm, SEED, count=st["count"], active=st["active"], limit=st["limit"], length=st["length"],
                          finish=st["finish"], stream=stream, allow=allow, ids_out=st["ids"], logprob_out=st["lp"], hist_ids=st["hid"],
                          hist_logits=st["hlg"], hist_logprob=st["hlp"], stop_mask=stop_mask, stop_seq=stop_seq, stop_frame=frame)


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("frame", [1, 3])
@pytest.mark.parametrize("S", [1, 5, 257])
def test_kernel_equals_the_rule_and_the_plain_sampler(S, frame, f32):
    top_k, top_p, temp = 4, 1.0, 1.0
    mask = acgt_mask()
    stop_bool = H.allowed_mask(None, STOP_TOKENS)
    allow, stop_mask = ops().pack_allow_mask(mask, DEV), ops().pack_allow_mask(stop_bool, DEV)
    stop_seq = ops().pack_stop_sequences(PATTERNS)
    prm = (torch.full((S,), top_k, dtype=torch.int32, device=DEV), torch.full((S,), top_p, dtype=torch.float32, device=DEV),
           torch.full((S,), temp, dtype=torch.float32, device=DEV))
    stream_cpu = torch.arange(S, dtype=torch.int64) * 3 + 1
    stream = stream_cpu.to(DEV)
    limit, active0, count0 = _initial(S)
    rows_cpu = _rows(S, f32, seed=S + frame)
    rows = rows_cpu.to(DEV)
    st = _state(S, limit, active0, count0)
    # the plain sampler's own outputs and histories, launched on exactly the rows that draw
    old = dict(ids=torch.full((S,), -7, dtype=torch.int64, device=DEV), lp=torch.full((S,), 123.0, dtype=torch.float32, device=DEV),
               hid=torch.full((S, L), -9, dtype=torch.int64, device=DEV), hlg=torch.full((S, L, 512), 777.0, dtype=torch.float32, device=DEV))
    # the specification's state
    w_count, w_active = count0.clone(), active0.clone()
    w_length, w_finish = torch.full((S,), -5, dtype=torch.int64), torch.full((S,), 9, dtype=torch.uint8)
    w_ids, w_hid = torch.full((S,), -7, dtype=torch.int64), torch.full((S, L), -9, dtype=torch.int64)
    w_lp, w_hlp = torch.full((S,), 123.0), torch.full((S, L), 777.0)
    w_hlg = torch.full((S, L, 512), 777.0)
    seen = set()
    for t in range(L):
        pre_count = w_count.clone()
        gone = w_active & ((w_count >= limit) | (w_count >= L))                     # ends by length without drawing
        draws = w_active & ~gone
        _launch(st, rows[t], prm, stream, allow, stop_mask, stop_seq, frame)
        ops().sample_rows(rows[t], *prm, SEED, stream=stream, count=pre_count.clone().to(DEV), allow=allow, active=draws.to(DEV),
                          ids_out=old["ids"], logprob_out=old["lp"], hist_ids=old["hid"], hist_logits=old["hlg"])
        torch.cuda.synchronize()
        for s in torch.nonzero(gone).flatten().tolist():
            w_active[s], w_length[s], w_finish[s] = False, w_count[s], H.FINISH_LENGTH
            seen.add((H.FINISH_LENGTH, "no draw"))
        d = torch.nonzero(draws).flatten()
        if len(d):
            toks = H.sample_seeded(rows_cpu[t][d].float(), top_k, top_p, temp, SEED, stream_cpu[d].numpy(), pre_count[d].numpy(), mask)
            for s, tok in zip(d.tolist(), toks.tolist()):
                cnt = int(pre_count[s])
                w_ids[s], w_hid[s, cnt], w_count[s] = tok, tok, cnt + 1
                w_hlg[s, cnt] = rows_cpu[t, s].float()
                fin = H.finish_reason(w_hid[s, : cnt + 1].tolist(), int(limit[s]), stop_bool, PATTERNS, frame)
                if fin:
                    w_active[s], w_length[s], w_finish[s] = False, cnt + 1, fin
                    seen.add((fin, cnt))
        got = {k: (v.cpu() if v is not None else None) for k, v in st.items()}
        assert torch.equal(got["ids"], w_ids), (t, torch.nonzero(got["ids"] != w_ids).flatten()[:8].tolist())
        assert torch.equal(got["count"], w_count) and torch.equal(got["active"], w_active), t
        assert torch.equal(got["length"], w_length) and torch.equal(got["finish"], w_finish), t
        assert torch.equal(got["hid"], w_hid), t
        # bit-identical to the plain sampler: token, log-probability (inactive and exhausted rows keep their canaries in both)
        assert torch.equal(got["ids"], old["ids"].cpu()) and torch.equal(got["lp"], old["lp"].cpu()), t
        w_lp[d] = got["lp"][d]
        w_hlp[d, pre_count[d]] = got["lp"][d]
        assert torch.equal(got["lp"], w_lp) and torch.equal(got["hlp"], w_hlp), t   # hist_logprob = logprob_out, canaries elsewhere
    assert torch.equal(got["hlg"], w_hlg) and torch.equal(got["hlg"], old["hlg"].cpu()) and torch.equal(got["hid"], old["hid"].cpu())
    assert not bool(w_active.any())                                                 # every job ended within its 12 launches
    if S >= 5:
        assert bool((got["ids"][4] == -7) and (got["hid"][4] == -9).all() and (got["hlg"][4] == 777.0).all() and got["finish"][4] == 9)
        want = {1: [(8, 2), (4, 2), (1, 2), (3, 1)], 3: [(12, 2), (11, 3), (3, 2), (3, 1)]}[frame]
        assert [(int(w_length[s]), int(w_finish[s])) for s in range(4)] == want
    if S == 1:
        assert (int(w_length[0]), int(w_finish[0])) == {1: (8, 2), 3: (12, 2)}[frame]
    if S == 257:
        # every reason at every count it can occur at: a stop token and the length at any n = cnt + 1, a pattern at any n in frame
        for cnt in range(L):
            assert (H.FINISH_STOP_TOKEN, cnt) in seen and (H.FINISH_LENGTH, cnt) in seen, (cnt, sorted(seen, key=str))
            if (cnt + 1) % frame == 0:
                assert (H.FINISH_STOP_SEQUENCE, cnt) in seen, (cnt, sorted(seen, key=str))
        assert (H.FINISH_LENGTH, "no draw") in seen
        assert int(got["length"][GONE_ROW]) == L and int(got["finish"][GONE_ROW]) == 3 and int(got["ids"][GONE_ROW]) == -7
    # the same 12 launches captured in one graph
    st2 = _state(S, limit, active0, count0)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for t in range(L):
            _launch(st2, rows[t], prm, stream, allow, stop_mask, stop_seq, frame)
    g.replay()
    torch.cuda.synchronize()
    for k, v in st.items():
        assert torch.equal(v, st2[k]), k


# ------------------------------------------------------------------------------------------------ arena
@covers("evo_sample_rows_ctl_f32")
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("hist", ["all", "ids", "none"])
def test_sample_rows_ctl_in_the_arena(hist, f32):
    """S = 5: a row at cnt = 0 under an 8-token pattern (nothing before its history may be read), a row in mid-history, an inactive row, a
    row with nothing left to draw, a row at the last cell.  `all`: the three histories; `ids`: the token history alone (the patterns need
    it); `none`: no history and no pattern -- stop token and limits only.  Per-row vectors at their element's alignment."""
    o, g = ops(), gen(5)
    S, Lh = 5, 9
    # (patterns ending in A and C: the row at the last cell looks back into its history, which holds the poison, for either token)
    stop_seq = o.pack_stop_sequences([[A, C, G, T, A, C, G, A], [C] * 8, [G]]) if hist != "none" else None
    inp = {"lg": rnd((S, 520), g, 3.0, torch.float32 if f32 else torch.bfloat16), "top_k": torch.full((S,), 4, dtype=torch.int32, device=DEV),
           "top_p": torch.full((S,), 0.9, dtype=torch.float32, device=DEV), "temp": torch.full((S,), 0.7, dtype=torch.float32, device=DEV),
           "stream": torch.arange(S, dtype=torch.int64, device=DEV) * 3 + 1,
           "count": torch.tensor([0, 2, 1, 4, Lh - 1], dtype=torch.int64, device=DEV),
           "active": torch.tensor([True, True, False, True, True], device=DEV),
           "limit": torch.tensor([9, 3, 9, 4, 9], dtype=torch.int64, device=DEV),
           "allow": o.pack_allow_mask(acgt_mask(), DEV), "stop_mask": o.pack_allow_mask(H.allowed_mask(None, [T]), DEV),
           "ids": poisoned((S,), torch.int64), "lp": poisoned((S,), torch.float32), "length": poisoned((S,), torch.int64),
           "finish": poisoned((S,), torch.uint8)}
    if hist != "none":
        inp["hist_ids"] = poisoned((S, Lh), torch.int64)
    if hist == "all":
        inp["hist_logits"] = poisoned((S, Lh, 512), torch.float32)
        inp["hist_logprob"] = poisoned((S, Lh), torch.float32)

    def fn(lg, top_k, top_p, temp, stream, count, active, limit, allow, stop_mask, ids, lp, length, finish, hist_ids=None, hist_logits=None,
           hist_logprob=None):
        o.sample_rows_ctl(lg[:, :512], top_k, top_p, temp, 1234, count=count, active=active, limit=limit, length=length, finish=finish,
                          stream=stream, allow=allow, ids_out=ids, logprob_out=lp, hist_ids=hist_ids, hist_logits=hist_logits,
                          hist_logprob=hist_logprob, stop_mask=stop_mask, stop_seq=stop_seq, stop_frame=1)
    run = _run(fn, inp, inout=["count", "active", "ids", "lp", "length", "finish"] + [k for k in inp if k.startswith("hist_")],
               expect=["evo_sample_rows_ctl_f32"],
               align={"top_k": 4, "top_p": 4, "temp": 4, "stream": 8, "count": 8, "active": 1, "limit": 8, "ids": 8, "lp": 4, "length": 8,
                      "finish": 1, "hist_ids": 8, "hist_logprob": 4})
    got = run.inputs
    from test_gpu_arena import is_poison
    assert got["count"].tolist() == [1, 3, 1, 4, Lh] and is_poison(got["ids"][2]) and is_poison(got["ids"][3]) and is_poison(got["lp"][3])
    assert got["active"].tolist()[1:] == [False] * 4                  # limit 3 reached, inactive, exhausted, last cell = limit 9
    assert int(got["length"][1]) == 3 and int(got["length"][3]) == 4 and int(got["length"][4]) == Lh and is_poison(got["length"][2])
    assert int(got["finish"][3]) == 3 and int(got["finish"][1]) in (1, 2, 3) and int(got["finish"][4]) in (1, 2, 3)
    if bool(got["active"][0]):
        assert is_poison(got["length"][0]) and is_poison(got["finish"][0])
    if hist != "none":
        hid = got["hist_ids"]
        assert int(hid[0, 0]) == int(got["ids"][0]) and int(hid[1, 2]) == int(got["ids"][1]) and int(hid[4, Lh - 1]) == int(got["ids"][4])
        assert is_poison(hid[2]) and is_poison(hid[3]) and is_poison(hid[0, 1:]) and is_poison(hid[4, : Lh - 1])
    if hist == "all":
        assert is_poison(got["hist_logits"][3]) and is_poison(got["hist_logits"][0, 1:]) and not is_poison(got["hist_logits"][0, 0])
        assert torch.equal(got["hist_logprob"][[0, 1, 4], [0, 2, Lh - 1]], got["lp"][[0, 1, 4]])


# ------------------------------------------------------------------------------------------------ pool
# Chosen on the GPU among N in {48, 96}, the sampling seed and the seed of the toy model's synthetic weights, for the conditions the prefix
# test asserts.  With the weights of seed 0 (and 1) every sample at T = 1.0 is a homopolymer run for every sampling seed tried (0 ... 11),
# so no stop codon can occur; the weights of seed 2 leave some variety: N = 96, sampling seed 4 gives 5 of 18 jobs a stop codon, 396 pooled
# steps against 475.
N_TOK, POOL_SEED, N_SPP, WEIGHTS_SEED = 96, 4, 3, 2
STOPS = dict(stop_sequences=["TAA", "TAG", "TGA"], stop_frame=3)
SET = dict(top_k=4, top_p=1.0, temperature=1.0)
_CACHE = {}


def pool_run(n_tokens=N_TOK, poll_every=8, use_graph=True, rule=True, **kw):
    """One pool run on the toy model: 4 slots, PROMPTS x 3, ACGT only.  Cached by its arguments (the runs are references to each other)."""
    from evo_amd.pool import DecodePool
    key = (str(n_tokens), poll_every, use_graph, rule, tuple(sorted(kw.items())))
    if key not in _CACHE:
        if "model" not in _CACHE:
            from evo_amd.tokenizer import CharLevelTokenizer
            cfgd = dict(SMALL4, use_interpolated_rotary_pos_emb=True, rotary_emb_scaling_factor=16)      # test_gpu_pool_seeded.make("toy")
            _CACHE["model"] = (build(cfgd, seed=WEIGHTS_SEED)[2], CharLevelTokenizer(512))
        m, tok = _CACHE["model"]
        gen_kw = {k: kw[k] for k in ("return_logits",) if k in kw}
        ctor_kw = {k: v for k, v in kw.items() if k not in gen_kw}
        pool = DecodePool(m, tok, n_slots=4, device=DEV, use_graph=use_graph, seed=POOL_SEED, allowed_tokens="ACGT", poll_every=poll_every,
                          **SET, **ctor_kw)
        out = pool.generate(PROMPTS, n_tokens=n_tokens, n_sample_per_prompt=N_SPP, **(STOPS if rule else {}), **gen_kw)
        _CACHE[key] = (pool,) + tuple(out)
    return _CACHE[key]


def test_pool_with_stop_codons_is_the_prefix_of_the_fixed_length_run():
    """Rests on a row's logits not depending on its slot or its neighbours at a fixed slot count (tests/test_gpu_pool_seeded.py asserts
    it for re-ordered prompts): a difference here would be a finding about row independence, not something for a tolerance."""
    F, seqs_f, _, _ = pool_run(rule=False)                             # today's path: evo_sample_rows_f32, every job N_TOK tokens
    Cp, seqs_c, scores_c, owner = pool_run()
    assert not hasattr(F, "last_lengths") and tuple(F.last_ids.shape) == (len(PROMPTS) * N_SPP, N_TOK)
    pats = H.stop_patterns(_CACHE["model"][1], STOPS["stop_sequences"])
    n_jobs = F.last_ids.shape[0]
    stops = 0
    for j in range(n_jobs):
        n, fin = H.stop_point(F.last_ids[j].tolist(), N_TOK, (), pats, 3)
        assert fin in (H.FINISH_STOP_SEQUENCE, H.FINISH_LENGTH)
        assert Cp.last_lengths[j] == n and Cp.last_finish[j] == H.FINISH_NAMES[fin], j
        assert torch.equal(Cp.last_ids[j, :n], F.last_ids[j, :n]) and bool((Cp.last_ids[j, n:] == -1).all()), j
        assert torch.equal(Cp.last_logits[j, :n], F.last_logits[j, :n]) and bool((Cp.last_logits[j, n:] == 0).all()), j
        assert seqs_c[j] == seqs_f[j][:n] and (fin == H.FINISH_LENGTH or seqs_c[j][-3:] in STOPS["stop_sequences"])
        stops += fin == H.FINISH_STOP_SEQUENCE
        # the fixed-length run keeps no log-probabilities: the plain sampler on its recorded rows, same stream and counts, gives the bits
        k = (torch.full((n,), SET["top_k"], dtype=torch.int32, device=DEV), torch.full((n,), SET["top_p"], dtype=torch.float32, device=DEV),
             torch.full((n,), SET["temperature"], dtype=torch.float32, device=DEV))
        ids, lp = ops().sample_rows(F.last_logits[j, :n].to(DEV), *k, POOL_SEED, stream=torch.full((n,), j, dtype=torch.int64, device=DEV),
                                    count=torch.arange(n, dtype=torch.int64, device=DEV), allow=F.s_allow)
        assert torch.equal(ids.cpu(), F.last_ids[j, :n]) and torch.equal(lp.cpu(), Cp.last_logprobs[j, :n]), j
        assert scores_c[j] == float(np.mean(lp.cpu().numpy().astype(np.float64)))
    print(f"[stop codons] {stops} of {n_jobs} jobs end by a stop codon, lengths {Cp.last_lengths}; steps {Cp.stats['steps']} against "
          f"{F.stats['steps']} at fixed length; polls {Cp.stats['polls']}, idle slot steps {Cp.stats['idle_slot_steps']}")
    assert 4 * stops >= n_jobs and stops < n_jobs                      # a quarter at least end by a stop, one at least by length
    assert Cp.stats["steps"] < F.stats["steps"]
    assert Cp.stats["stop_ends"] == stops and Cp.stats["length_ends"] == n_jobs - stops
    assert Cp.stats["tokens"] == sum(Cp.last_lengths) - n_jobs
    # the poll interval and the graph change nothing
    for other in (pool_run(poll_every=1), pool_run(use_graph=False)):
        P = other[0]
        assert other[1] == seqs_c and other[2] == scores_c and P.last_lengths == Cp.last_lengths and P.last_finish == Cp.last_finish
        assert torch.equal(P.last_ids, Cp.last_ids) and torch.equal(P.last_logprobs, Cp.last_logprobs)
        assert torch.equal(P.last_logits, Cp.last_logits)


def test_stop_tokens_on_one_graph_pool_called_again_and_again():
    """One pool, its step captured once, three generate() calls: stop token T, stop token A (another rule under the same captured launch:
    the stop mask is per-pool state the rule is copied into), T again.  Each run is the prefix of the fixed-length run that its own rule
    cuts out, the stop token trimmed from the string."""
    from evo_amd.pool import DecodePool
    F, seqs_f, _, _ = pool_run(rule=False)
    m, tok = _CACHE["model"]
    pool = DecodePool(m, tok, n_slots=4, device=DEV, use_graph=True, seed=POOL_SEED, allowed_tokens="ACGT", **SET)
    n_jobs = F.last_ids.shape[0]
    runs = []
    for stop in ("T", "A", "T"):
        seqs, scores, _ = pool.generate(PROMPTS, n_tokens=N_TOK, n_sample_per_prompt=N_SPP, stop_tokens=stop)
        graph = pool._graph
        assert graph is not None and (not runs or graph is runs[-1][0])              # captured once, replayed by every later call
        stop_set = {ord(stop)}
        for j in range(n_jobs):
            n, fin = H.stop_point(F.last_ids[j].tolist(), N_TOK, stop_set, (), 1)
            assert pool.last_lengths[j] == n and pool.last_finish[j] == H.FINISH_NAMES[fin], (stop, j)
            assert torch.equal(pool.last_ids[j, :n], F.last_ids[j, :n]) and torch.equal(pool.last_logits[j, :n], F.last_logits[j, :n]), (stop, j)
            assert seqs[j] == (seqs_f[j][: n - 1] if fin == H.FINISH_STOP_TOKEN else seqs_f[j][:n]) and stop not in seqs[j]
        print(f"[stop token {stop}] lengths {pool.last_lengths}, polls {pool.stats['polls']}, idle slot steps {pool.stats['idle_slot_steps']}")
        assert "stop_token" in pool.last_finish
        runs.append((graph, seqs, scores, pool.last_ids.clone(), pool.last_logprobs.clone()))
    assert runs[0][1] != runs[1][1]                                                  # the two rules cut differently
    assert runs[0][1] == runs[2][1] and runs[0][2] == runs[2][2] and torch.equal(runs[0][3], runs[2][3]) and torch.equal(runs[0][4], runs[2][4])
    assert not bool(pool.s_active.any())
    # a fixed-length call on the same pool: the job-control attributes of the earlier run are gone
    pool.generate(PROMPTS[:2], n_tokens=4)
    assert not hasattr(pool, "last_lengths") and not hasattr(pool, "last_finish") and not hasattr(pool, "last_logprobs")


MIX = [40] + [3] * (len(PROMPTS) - 1)


@pytest.mark.parametrize("rule", ["codons", "limits"])
@pytest.mark.parametrize("option", ["share_prompt_kv", "prefill_batch"])
def test_pool_combinations(option, rule):
    """share_prompt_kv / prefill_batch change the attention and prefill kernels: nothing is compared across paths.  Every token is the
    specification's draw from its own recorded logits (the acceptance rule of tests/test_gpu_sample.py that `accepted` of
    tests/test_gpu_pool_seeded.py applies -- called here on the jobs' own lengths, which that helper's fixed 24 columns cannot hold), and
    the rule applied to the job's own tokens gives its length and finish."""
    kw = {"share_prompt_kv": True} if option == "share_prompt_kv" else {"prefill_batch": 4}
    n_tokens = N_TOK if rule == "codons" else tuple(MIX)
    P, seqs, scores, owner = pool_run(n_tokens=n_tokens, rule=rule == "codons", **kw)
    pats = H.stop_patterns(_CACHE["model"][1], STOPS["stop_sequences"]) if rule == "codons" else []
    n_jobs = len(owner)
    rows, toks, st, ct = [], [], [], []
    for j in range(n_jobs):
        n = P.last_lengths[j]
        lim = N_TOK if rule == "codons" else MIX[owner[j]]
        assert (n, H.FINISH_NAMES[H.finish_reason(P.last_ids[j, :n].tolist(), lim, (), pats, 3)]) == \
            H.stop_point(P.last_ids[j, :n].tolist(), lim, (), pats, 3)[:1] + (P.last_finish[j],), j
        assert bool((P.last_ids[j, n:] == -1).all()) and len(seqs[j]) == n
        rows.append(P.last_logits[j, :n])
        toks.append(P.last_ids[j, :n])
        st.append(np.full(n, j))
        ct.append(np.arange(n))
    out, bad = accept(torch.cat(rows), torch.cat(toks), SET["top_k"], SET["top_p"], SET["temperature"], acgt_mask(), POOL_SEED,
                      np.concatenate(st), np.concatenate(ct))
    assert out.float().mean().item() <= 0.04 and int(bad.sum()) == 0
    if rule == "limits":
        assert P.last_lengths == [MIX[o] for o in owner] and P.stats["polls"] == 0
    print(f"[stop combinations {option} {rule}] lengths {P.last_lengths}, finish {sorted(set(P.last_finish))}")
    if option == "share_prompt_kv":
        R = min(4, len(PROMPTS))
        assert P.stats["store_rows"] == R and P.store_refs == [0] * R and P.store.row.tolist() == [-1] * 4
    else:
        assert P.stats["prefills"] < len(PROMPTS)
    assert not bool(P.s_active.any())
    # two runs are identical
    from evo_amd.pool import DecodePool
    m, tok = _CACHE["model"]
    Q = DecodePool(m, tok, n_slots=4, device=DEV, use_graph=True, seed=POOL_SEED, allowed_tokens="ACGT", **SET, **kw)
    seqs_q, scores_q, _ = Q.generate(PROMPTS, n_tokens=list(n_tokens) if rule == "limits" else n_tokens, n_sample_per_prompt=N_SPP,
                                     **(STOPS if rule == "codons" else {}))
    assert seqs_q == seqs and scores_q == scores and torch.equal(Q.last_ids, P.last_ids) and torch.equal(Q.last_logits, P.last_logits)
    assert torch.equal(Q.last_logprobs, P.last_logprobs) and Q.last_finish == P.last_finish


def test_scores_and_the_run_without_logits():
    P, seqs, scores, _ = pool_run()
    # fp64 yardstick; tolerance 4 x the error of the same formula restated in fp32 torch, on the same rows (tests/test_gpu_sample.py)
    err = err32 = 0.0
    for j, n in enumerate(P.last_lengths):
        x = P.last_logits[j, :n]
        t = P.last_ids[j, :n, None]
        ref = torch.log_softmax(x.double(), -1).gather(-1, t)[:, 0]
        mx = x.max(-1, keepdim=True)[0]
        lsm32 = (x - (mx + (x - mx).exp().sum(-1, keepdim=True).log())).gather(-1, t)[:, 0]
        err = max(err, abs(scores[j] - ref.mean().item()), (P.last_logprobs[j, :n].double() - ref).abs().max().item())
        err32 = max(err32, (lsm32.double() - ref).abs().max().item())
    print(f"[stop scores] max |err| {err:.3e}, fp32 torch restatement {err32:.3e}")
    assert err <= 4 * err32, (err, err32)
    Q, seqs_q, scores_q, _ = pool_run(return_logits=False)
    assert Q.last_logits is None and Q.hist_logits is None
    assert seqs_q == seqs and scores_q == scores and torch.equal(Q.last_ids, P.last_ids) and torch.equal(Q.last_logprobs, P.last_logprobs)
    assert Q.last_lengths == P.last_lengths and Q.last_finish == P.last_finish
