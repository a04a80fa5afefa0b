"""CPU: decode-pool jobs that end on their own -- the layers that need no GPU.

  * the written rule (evo_amd/sh/sample.py: finish_reason, stop_point, sample_ctl, stop_patterns, pack_stop_sequences): priority of the
    reasons, frame gating, a pattern longer than the tokens there are, a job that ends on its first token;
  * the C entry evo_sample_rows_ctl_f32: exported, declared, bound, ABI 17, and every contract violation of include/evo_mi355x.h refused
    with -1 before any launch (null or never-dereferenced pointers; the stop patterns are HOST arrays, so their lengths are checked here);
  * the scheduler of DecodePool on the fp64 oracle backend, with `sample_rows` / `sample_rows_ctl` written from the specification: every
    job equals a one-job-at-a-time loop written here, every store row is released, `poll_every` changes nothing but the number of reads,
    and without a stop rule nothing is read at all;
  * resources: the control kernel without scratch or spills, in the LDS of the kernel it shares its draw with (the patterns travel in the
    launch's arguments: no LDS of their own)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from evo_amd import _build
from evo_amd import ops as evo_ops
from evo_amd.pool import DecodePool, sample_many
from evo_amd.sh import sample as H
from evo_amd.tokenizer import CharLevelTokenizer
from test_fanout_host import SMALL, FanoutOracleOps
from test_gpu_pool import PROMPTS
from test_kernel_resources import HIPCC, _metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOK = CharLevelTokenizer(512)
A, C, G, T = (ord(c) for c in "ACGT")
CODONS = [[T, A, A], [T, A, G], [T, G, A]]


# ------------------------------------------------------------------------------------------------ the rule
def test_priority_of_the_reasons():
    stop = {G}
    # a stop token that also completes a pattern at the limit: the stop token wins
    assert H.finish_reason([T, A, G], 3, stop, CODONS, 3) == H.FINISH_STOP_TOKEN
    # a pattern completed at the limit: the pattern wins over the length
    assert H.finish_reason([T, A, A], 3, stop, CODONS, 3) == H.FINISH_STOP_SEQUENCE
    assert H.finish_reason([C, A, A], 3, stop, CODONS, 3) == H.FINISH_LENGTH
    assert H.finish_reason([C, A, A], 4, stop, CODONS, 3) == H.FINISH_RUNNING
    assert H.finish_reason([C, A, A, T], 3, (), (), 1) == H.FINISH_LENGTH           # n beyond the limit still ends by length
    mask = torch.zeros(512, dtype=torch.bool)
    mask[G] = True
    assert H.finish_reason([T, A, G], 9, mask, (), 1) == H.FINISH_STOP_TOKEN         # the set as a mask
    assert H.finish_reason([T, A, A], 9, mask, (), 1) == H.FINISH_RUNNING
    assert H.FINISH_NAMES == {1: "stop_token", 2: "stop_sequence", 3: "length"}
    with pytest.raises(ValueError):
        H.finish_reason([A], 3, (), (), 0)


def test_frame_gating_counts_from_the_first_generated_token():
    assert H.finish_reason([C, T, A, A], 99, (), CODONS, 3) == H.FINISH_RUNNING      # TAA ending at n = 4: out of frame
    assert H.finish_reason([C, T, A, A], 99, (), CODONS, 1) == H.FINISH_STOP_SEQUENCE
    assert H.finish_reason([C, T, A, A], 99, (), CODONS, 2) == H.FINISH_STOP_SEQUENCE
    assert H.finish_reason([C, C, C, T, A, A], 99, (), CODONS, 3) == H.FINISH_STOP_SEQUENCE
    assert H.stop_point([C, T, A, A, C, G, T, G, A, C], 99, (), CODONS, 3) == (9, H.FINISH_STOP_SEQUENCE)
    assert H.stop_point([C, T, A, A, C, G, T, G, A, C], 8, (), CODONS, 3) == (8, H.FINISH_LENGTH)
    assert H.stop_point([C, T, A], 8, (), CODONS, 3) == (3, H.FINISH_RUNNING)       # the tokens ran out first


def test_a_pattern_longer_than_the_tokens_reads_nothing():
    long = [[A, C, G, T, A, C, G, T]]
    for n in range(1, 8):
        assert H.finish_reason([A, C, G, T, A, C, G][-n:] + [T], 99, (), long, 1) == (H.FINISH_STOP_SEQUENCE if n == 7 else H.FINISH_RUNNING)
    assert H.finish_reason([T], 99, (), long + [[T]], 1) == H.FINISH_STOP_SEQUENCE  # a 1-token pattern on the first token
    # the comparison never wraps to the other end of the list
    assert H.finish_reason([T, A], 99, (), [[A, T, A]], 1) == H.FINISH_RUNNING


def test_limit_one_ends_on_the_first_token_and_an_exhausted_row_draws_nothing():
    row = torch.randn(512, generator=torch.Generator().manual_seed(0))
    want = int(H.sample_seeded(row, 4, 1.0, 1.0, 5, 7, 0))
    assert H.sample_ctl(row, 4, 1.0, 1.0, 5, 7, [], 1) == (want, 1, H.FINISH_LENGTH)
    assert H.sample_ctl(row, 4, 1.0, 1.0, 5, 7, [], 2) == (want, 1, H.FINISH_RUNNING)
    assert H.sample_ctl(row, 4, 1.0, 1.0, 5, 7, [], 9, stop_tokens={want}) == (want, 1, H.FINISH_STOP_TOKEN)
    assert H.sample_ctl(row, 4, 1.0, 1.0, 5, 7, [], 9, stop_sequences=[[want]]) == (want, 1, H.FINISH_STOP_SEQUENCE)
    nxt = int(H.sample_seeded(row, 4, 1.0, 1.0, 5, 7, 2))                          # draw number = tokens recorded
    assert H.sample_ctl(row, 4, 1.0, 1.0, 5, 7, [A, C], 9)[0] == nxt
    assert H.sample_ctl(row, 4, 1.0, 1.0, 5, 7, [A, C], 2) == (None, 2, H.FINISH_LENGTH)
    assert H.sample_ctl(row, 4, 1.0, 1.0, 5, 7, [A, C], 9, hist_len=2) == (None, 2, H.FINISH_LENGTH)


def test_patterns_are_validated_and_packed():
    assert H.stop_patterns(TOK, ["TAA", "TAG", "TGA"]) == CODONS
    assert H.stop_patterns(TOK, "TAA") == [[T, A, A]] and H.stop_patterns(TOK, None) == []
    assert H.stop_patterns(TOK, [[1, 2], torch.tensor([3])]) == [[1, 2], [3]]
    for bad in ([""], [[]], ["ACGTACGTA"], ["A"] * 9, [[512]], [[-1]]):
        with pytest.raises(ValueError):
            H.stop_patterns(TOK, bad)
    seq, ln = evo_ops.HipOps.pack_stop_sequences(CODONS + [[G]])
    assert seq.dtype == ln.dtype == torch.int32 and tuple(seq.shape) == (4, 8) and ln.tolist() == [3, 3, 3, 1]
    assert seq[1].tolist() == [T, A, G] + [-1] * 5 and seq[3, 0] == G
    seq0, ln0 = H.pack_stop_sequences([])
    assert tuple(seq0.shape) == (0, 8) and ln0.numel() == 0


# ------------------------------------------------------------------------------------------------ C ABI
def test_the_entry_is_exported_and_refuses_before_any_launch():
    header = open(os.path.join(ROOT, "include", "evo_mi355x.h")).read()
    name = "evo_sample_rows_ctl_f32"
    assert name in _build.EXPORTS and name in evo_ops._SIGNATURES and re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert int(re.search(r"#define EVO_ABI_VERSION (\d+)", header).group(1)) == evo_ops.ABI_VERSION >= 17
    assert hasattr(evo_ops.HipOps, "sample_rows_ctl") and hasattr(evo_ops.HipOps, "pack_stop_sequences")
    lib = evo_ops.load_library()
    assert lib.evo_abi_version() == evo_ops.ABI_VERSION
    f = lib.evo_sample_rows_ctl_f32
    one = ctypes.c_void_p(16)                                         # (non-null, 16-byte aligned, never dereferenced)
    seq, ln = H.pack_stop_sequences(CODONS)                           # host arrays: these ARE read by the entry
    names = ["logits", "logits_f32", "ld", "top_k", "top_p", "temperature", "allow", "seed", "stream_id", "count", "active", "ids_out",
             "logprob_out", "hist_ids", "hist_logits", "hist_logprob", "hist_len", "limit", "stop_mask", "stop_seq", "stop_seq_len", "n_seq",
             "stop_frame", "length", "finish", "S", "V", "stream"]
    ok = dict(logits=one, logits_f32=0, ld=512, top_k=one, top_p=one, temperature=one, allow=None, seed=1, stream_id=None, count=one,
              active=one, ids_out=one, logprob_out=one, hist_ids=one, hist_logits=None, hist_logprob=None, hist_len=8, limit=one,
              stop_mask=None, stop_seq=seq.data_ptr(), stop_seq_len=ln.data_ptr(), n_seq=3, stop_frame=3, length=one, finish=one, S=4, V=512,
              stream=None)
    assert list(ok) == names and len(evo_ops._SIGNATURES[name][0]) == len(names)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return f(*[a[n] for n in names])
    for n in ("count", "active", "limit", "length", "finish"):
        assert call(**{n: None}) == -1, n                             # what job control needs
    for n in ("logits", "top_k", "top_p", "temperature", "ids_out", "logprob_out"):
        assert call(**{n: None}) == -1, n                             # what evo_sample_rows_f32 refuses
    assert call(S=0) == -1 and call(V=256) == -1 and call(ld=500) == -1 and call(ld=516) == -1
    assert call(logits=ctypes.c_void_p(8)) == -1 and call(hist_logits=ctypes.c_void_p(24)) == -1
    assert call(hist_len=0) == -1                                     # a history without room
    assert call(hist_ids=None, n_seq=0, hist_logprob=one, hist_len=0) == -1
    nine = torch.full((9, 8), A, dtype=torch.int32)
    nine_len = torch.full((9,), 3, dtype=torch.int32)
    assert call(stop_seq=nine.data_ptr(), stop_seq_len=nine_len.data_ptr(), n_seq=9) == -1       # more than 8 patterns
    assert call(n_seq=-1) == -1
    for bad in (0, 9, -3):
        bad_len = torch.tensor([3, bad, 3], dtype=torch.int32)
        assert call(stop_seq_len=bad_len.data_ptr()) == -1, bad       # a pattern length outside 1 ... 8
    assert call(hist_ids=None, hist_logprob=one) == -1                # patterns without the token history they look back into
    assert call(stop_seq=None) == -1 and call(stop_seq_len=None) == -1
    assert call(stop_frame=0) == -1 and call(stop_frame=-3) == -1


# ------------------------------------------------------------------------------------------------ the scheduler on the oracle backend
def _bits(packed):
    return None if packed is None else ((packed.cpu().to(torch.int32)[:, None] >> torch.arange(8, dtype=torch.int32)[None, :]) & 1).bool().reshape(512)


class CtlOracleOps(FanoutOracleOps):
    """The oracle backend + both sampler launches, row by row from the written specification."""
    pack_allow_mask = staticmethod(evo_ops.HipOps.pack_allow_mask)
    pack_stop_sequences = staticmethod(H.pack_stop_sequences)

    def sample_rows(self, logits, top_k, top_p, temperature, seed, stream=None, count=None, allow=None, active=None, ids_out=None,
                    logprob_out=None, hist_ids=None, hist_logits=None):
        for s in range(logits.shape[0]):
            if active is not None and not bool(active[s]):
                continue
            cnt = int(count[s])
            tok = int(H.sample_seeded(logits[s], int(top_k[s]), float(top_p[s]), float(temperature[s]), seed, int(stream[s]), cnt, _bits(allow)))
            ids_out.view(-1)[s] = tok
            logprob_out[s] = torch.log_softmax(logits[s].double(), -1)[tok]
            if 0 <= cnt < hist_ids.shape[1]:
                hist_ids[s, cnt] = tok
                hist_logits[s, cnt] = logits[s].float()
            count[s] = cnt + 1

    def sample_rows_ctl(self, logits, top_k, top_p, temperature, seed, count, active, limit, length, finish, stream=None, allow=None,
                        ids_out=None, logprob_out=None, hist_ids=None, hist_logits=None, hist_logprob=None, stop_mask=None, stop_seq=None,
                        stop_frame=1):
        pats = [] if stop_seq is None else [stop_seq[0][q, : int(stop_seq[1][q])].tolist() for q in range(len(stop_seq[1]))]
        for s in range(logits.shape[0]):
            if not bool(active[s]):
                continue
            cnt = int(count[s])
            tok, n, fin = H.sample_ctl(logits[s], int(top_k[s]), float(top_p[s]), float(temperature[s]), seed, int(stream[s]),
                                       hist_ids[s, :cnt].tolist(), int(limit[s]), _bits(allow), _bits(stop_mask), pats, stop_frame,
                                       hist_len=hist_ids.shape[1])
            if tok is not None:
                ids_out.view(-1)[s] = tok
                lp = torch.log_softmax(logits[s].double(), -1)[tok]
                logprob_out[s] = lp
                hist_ids[s, cnt] = tok
                hist_logprob[s, cnt] = lp
                if hist_logits is not None:
                    hist_logits[s, cnt] = logits[s].float()
                count[s] = n
            if fin:
                active[s], length[s], finish[s] = False, n, fin


@pytest.fixture(scope="module")
def small():
    from oracle.stripedhyena_ref import RefConfig, make_synthetic_state_dict
    from evo_amd.sh.model import StripedHyena
    sd = make_synthetic_state_dict(RefConfig.from_dict(SMALL), seed=3)
    m = StripedHyena(dict(SMALL), ops=CtlOracleOps(torch.float64))
    m.load_state_dict({k: (v.double() if v.dtype == torch.bfloat16 else v) for k, v in sd.items()})
    return m


SEED, TOP_K, TEMP, N_SPP = 11, 4, 10.0, 2                            # (the synthetic model repeats its last token: T = 10 spreads the draws)
MIX = [40] + [3] * (len(PROMPTS) - 1)                                 # prompt 0 outlives every other job
RULES = {"limits": dict(limits=MIX), "codons": dict(limits=[12] * len(PROMPTS), stop_sequences=["TA", "GG", "CAC"], stop_frame=2),
         "token": dict(limits=MIX, stop_tokens="G")}
_NAIVE = {}


def naive(m, rule):
    """One job at a time, every token from a full forward of (prompt + tokens so far): [(ids, logprobs, finish)] in job order."""
    if rule in _NAIVE:
        return _NAIVE[rule]
    r = RULES[rule]
    allow = H.allowed_mask(TOK, "ACGT")
    stop = H.allowed_mask(TOK, r["stop_tokens"]) if "stop_tokens" in r else None
    pats = H.stop_patterns(TOK, r.get("stop_sequences"))
    out = []
    with torch.inference_mode():
        for pi, p in enumerate(PROMPTS):
            for c in range(N_SPP):
                hist, lps, fin = [], [], 0
                while not fin:
                    row = m(torch.tensor([list(p.encode()) + hist]))[0][0, -1].double()
                    tok, n, fin = H.sample_ctl(row, TOP_K, 1.0, TEMP, SEED, pi * N_SPP + c, hist, r["limits"][pi], allow, stop, pats,
                                               r.get("stop_frame", 1))
                    hist.append(tok)
                    lps.append(float(torch.log_softmax(row, -1)[tok]))
                out.append((hist, lps, fin))
    _NAIVE[rule] = out
    return out


def run_pool(m, rule, n_slots, share, poll_every=8, **kw):
    r = RULES[rule]
    pool = DecodePool(m, TOK, n_slots=n_slots, top_k=TOP_K, top_p=1.0, temperature=TEMP, device="cpu", seed=SEED, allowed_tokens="ACGT",
                      share_prompt_kv=share, poll_every=poll_every)
    gen = {k: r[k] for k in ("stop_tokens", "stop_sequences", "stop_frame") if k in r}
    seqs, scores, owner = pool.generate(PROMPTS, n_tokens=r["limits"], n_sample_per_prompt=N_SPP, **gen, **kw)
    return pool, seqs, scores, owner


def check_against_naive(pool, seqs, scores, owner, want):
    assert owner == [pi for pi in range(len(PROMPTS)) for _ in range(N_SPP)]
    assert pool.last_lengths == [len(h) for h, _, _ in want]
    assert pool.last_finish == [H.FINISH_NAMES[f] for _, _, f in want]
    for j, (hist, lps, fin) in enumerate(want):
        n = len(hist)
        assert pool.last_ids[j, :n].tolist() == hist and (pool.last_ids[j, n:] == -1).all(), j
        # the oracle sampler stores the fp64 log-probability in f32: within one ulp (2^-19) of a value below 32 in magnitude
        assert max(abs(x) for x in lps) < 32 and np.allclose(pool.last_logprobs[j, :n].numpy(), lps, rtol=0, atol=2.0 ** -19), j
        assert abs(scores[j] - float(np.mean(lps))) <= 2.0 ** -19
        text = "".join(chr(t) for t in hist)
        assert seqs[j] == (text[:-1] if fin == H.FINISH_STOP_TOKEN else text)


@pytest.mark.parametrize("share", [False, True], ids=["replicated", "shared"])
@pytest.mark.parametrize("n_slots", [2, 4])
def test_per_prompt_limits_one_job_outlives_the_rest(small, n_slots, share):
    want = naive(small, "limits")
    pool, seqs, scores, owner = run_pool(small, "limits", n_slots, share)
    check_against_naive(pool, seqs, scores, owner, want)
    assert [len(s) for s in seqs] == [40, 40] + [3] * 10 and pool.last_finish == ["length"] * 12
    assert pool.stats["polls"] == 0 and pool.stats["idle_slot_steps"] == 0          # no stop rule: the host knows every end by itself
    assert pool.stats["length_ends"] == 12 and pool.stats["stop_ends"] == 0
    assert pool.stats["tokens"] == sum(pool.last_lengths) - 12
    assert pool.last_logits is not None and tuple(pool.last_logits.shape) == (12, 40, 512)
    assert bool((pool.last_logits[2:, 3:] == 0).all()) and bool((pool.last_logits[:2] != 0).any(-1).all())
    if share:
        R = min(n_slots, len(PROMPTS))
        assert pool.stats["store_rows"] == R == len(pool.store_refs)
        assert pool.store_refs == [0] * R and pool.store.row.tolist() == [-1] * n_slots       # every store row released
        assert pool.stats["prompt_kv_installs"] == len(PROMPTS)
    assert not bool(pool.s_active.any())


@pytest.mark.parametrize("rule", ["codons", "token"])
@pytest.mark.parametrize("n_slots,share", [(2, True), (4, False), (4, True)])
def test_stop_rules_and_the_poll_interval(small, rule, n_slots, share):
    want = naive(small, rule)
    runs = [run_pool(small, rule, n_slots, share, poll_every=pe) for pe in (1, 8)]
    for pool, seqs, scores, owner in runs:
        check_against_naive(pool, seqs, scores, owner, want)
        assert pool.stats["stop_ends"] + pool.stats["length_ends"] == 12 and pool.stats["stop_ends"] >= 3
        assert pool.stats["polls"] > 0
        assert pool.stats["tokens"] == sum(pool.last_lengths) - 12
        if share:
            assert pool.store_refs == [0] * len(pool.store_refs) and pool.store.row.tolist() == [-1] * n_slots
    (p1, s1, sc1, _), (p8, s8, sc8, _) = runs
    assert s1 == s8 and sc1 == sc8 and torch.equal(p1.last_ids, p8.last_ids) and torch.equal(p1.last_logprobs, p8.last_logprobs)
    assert torch.equal(p1.last_logits, p8.last_logits)
    # a look after every step and after every round of fills (a job may end on its first token, drawn when its slot was filled):
    # nobody waits
    assert p1.stats["idle_slot_steps"] == 0 <= p8.stats["idle_slot_steps"] and p1.stats["polls"] >= p8.stats["polls"]
    assert p8.stats["steps"] >= p1.stats["steps"]
    if rule == "token":
        assert any(f == "stop_token" for f in p1.last_finish) and all("G" not in s for s in s1)
    else:
        assert any(f == "stop_sequence" for f in p1.last_finish)


def test_scores_only_other_arguments_and_what_is_refused(small):
    want = naive(small, "codons")
    pool, seqs, scores, owner = run_pool(small, "codons", 4, True, return_logits=False)
    check_against_naive(pool, seqs, scores, owner, want)
    assert pool.last_logits is None and pool.hist_logits is None
    # the same pool, then the fixed-length path on it, then job control again: each captures / allocates what it needs
    fixed = DecodePool(small, TOK, n_slots=4, top_k=TOP_K, top_p=1.0, temperature=TEMP, device="cpu", seed=SEED, allowed_tokens="ACGT")
    f_seqs, f_scores, _ = fixed.generate(PROMPTS, n_tokens=3, n_sample_per_prompt=N_SPP)
    p_seqs, p_scores, _ = pool.generate(PROMPTS, n_tokens=3, n_sample_per_prompt=N_SPP)
    assert p_seqs == f_seqs and p_scores == f_scores and pool.last_logits is not None
    assert not hasattr(pool, "last_lengths") and not hasattr(pool, "last_finish") and not hasattr(pool, "last_logprobs")
    again = pool.generate(PROMPTS, n_tokens=[12] * len(PROMPTS), n_sample_per_prompt=N_SPP, stop_sequences=["TA", "GG", "CAC"], stop_frame=2)
    assert again[0] == seqs and again[1] == scores
    # a pool made without seed or mask: job control moves the sampler onto the device with seed 0 for that call only
    plain = DecodePool(small, TOK, n_slots=2, top_k=1, device="cpu")
    s0, _, _ = plain.generate(PROMPTS[:2], n_tokens=[2, 4])
    assert [len(s) for s in s0] == [2, 4] and not plain.device_sampler
    # sample_many passes the arguments through
    _, sm_seqs, sm_scores = sample_many(PROMPTS, small, TOK, n_tokens=12, temp=TEMP, top_k=TOP_K, n_sample_per_prompt=N_SPP, n_slots=4,
                                        device="cpu", seed=SEED, allowed_tokens="ACGT", stop_sequences=["TA", "GG", "CAC"], stop_frame=2,
                                        return_logits=False, poll_every=3)
    assert sm_seqs == seqs and sm_scores == scores
    mk = lambda **kw: DecodePool(small, TOK, n_slots=2, device="cpu", seed=1, **kw)
    with pytest.raises(ValueError, match="outside allowed_tokens"):
        mk(allowed_tokens="ACGT").generate(PROMPTS[:1], n_tokens=4, stop_tokens="N")
    with pytest.raises(ValueError, match="at most 8"):
        mk().generate(PROMPTS[:1], n_tokens=4, stop_sequences=["A"] * 9)
    for bad in ([""], ["ACGTACGTA"]):
        with pytest.raises(ValueError, match="1 to 8 tokens"):
            mk().generate(PROMPTS[:1], n_tokens=4, stop_sequences=bad)
    with pytest.raises(ValueError):
        mk().generate(PROMPTS[:2], n_tokens=[4])
    with pytest.raises(ValueError):
        mk().generate(PROMPTS[:1], n_tokens=4, stop_frame=0)
    with pytest.raises(ValueError):
        DecodePool(small, TOK, n_slots=2, device="cpu", poll_every=0)


# ------------------------------------------------------------------------------------------------ resources
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_control_kernel_needs_no_scratch_and_no_more_lds():
    meta = _metadata("sample.hip")
    old = [v for k, v in meta.items() if "sample_rows_kernel" in k]
    new = [v for k, v in meta.items() if "sample_rows_ctl_kernel" in k]
    assert len(old) == 1 and len(new) == 1, sorted(meta)
    print("sample_rows_kernel", old[0], "sample_rows_ctl_kernel", new[0])
    for r in old + new:
        assert r["scratch"] == 0 and r["spill"] == 0 and r["sgpr_spill"] == 0, r
    assert new[0]["lds"] <= old[0]["lds"]                             # the patterns are launch arguments: no LDS of their own
