"""CPU: k-mer repeat control of the decode pool -- the layers that need no GPU.

  * wiring: the C entry evo_repeat_rows_f32 exported, declared, bound, ABI still 20, the optional group "repeat", the argument on
    DecodePool.generate / sample_many, the CLI flags; every contract violation refused with -1 before any launch (the pointers passed are
    never dereferenced);
  * the written rule (evo_amd/sh/sample.py: repeat_fold / repeat_init / repeat_penalise / repeat_ended) on hand-made cases;
  * the pool on the fp64 oracle backend with `repeat_rows` written from the rule (RepeatOracleOps): zero levels change nothing, the
    device's statistics equal a host recount, jobs end where the rule replayed on their tokens ends them, a huge level forbids what it
    should, and the launch composes with a stop sequence and a constraint;
  * what is refused, before any forward."""
import ctypes
import inspect
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
from evo_amd.pool import DecodePool, sample_many
from evo_amd.sh import sample as H
from evo_amd.sh.sample import RepeatControl, RepeatState
from test_paged_kv_host import PagedCtlOps, _model
from test_stop_host import PROMPTS, TOK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, C, G, T = (ord(c) for c in "ACGT")
ACGT = (A, C, G, T)
NAME = "evo_repeat_rows_f32"


# ------------------------------------------------------------------------------------------------ wiring and the C ABI
def test_the_entry_is_wired():
    header = open(os.path.join(ROOT, "include", "evo_mi355x.h")).read()
    assert NAME in _build.EXPORTS and NAME in evo_ops._SIGNATURES and re.search(r"\bint\s+" + NAME + r"\s*\(", header)
    assert int(re.search(r"#define EVO_ABI_VERSION (\d+)", header).group(1)) == evo_ops.ABI_VERSION == 20     # additive: no signature changed
    assert evo_ops.load_library().evo_abi_version() == 20
    assert int(re.search(r"#define EVO_FINISH_REPEAT (\d+)", header).group(1)) == H.FINISH_REPEAT == 6
    assert Backend.OPTIONAL["repeat"] == ("repeat_rows",) and hasattr(evo_ops.HipOps, "repeat_rows")
    assert any(p.name == "repeat.hip" for p in _build.sources())
    assert evo_amd.RepeatControl is RepeatControl
    for fn in (DecodePool.generate, sample_many):
        assert "repeat" in inspect.signature(fn).parameters
    text = open(os.path.join(ROOT, "scripts", "sample_many.py")).read()
    for flag in ("--repeat-k", "--repeat-penalty", "--repeat-max-count", "--repeat-ignore-prompt", "--repeat-end-fraction",
                 "--repeat-end-min-tokens"):
        assert flag in text, flag
    # the older mappings are what they were; the new one adds one name
    assert H.FINISH_NAMES == {1: "stop_token", 2: "stop_sequence", 3: "length"}
    assert H.FINISH_NAMES_ALL == {**H.FINISH_NAMES, 4: "constraint", 5: "dead_end"}
    assert H.FINISH_NAMES_REPEAT == {**H.FINISH_NAMES_ALL, 6: "repeat"}


def test_the_entry_refuses_before_any_launch():
    f = getattr(evo_ops.load_library(), NAME)
    ONE = ctypes.c_void_p(16)                                         # non-null, 16-byte aligned, never dereferenced
    alpha = torch.tensor(ACGT, dtype=torch.int32)                    # a host array: this IS read by the entry
    names = ["logits", "logits_f32", "ld", "out", "fed_ids", "active", "counts", "ctx", "stat", "levels", "end_num", "end_min_tokens", "count",
             "length", "finish", "alphabet", "n_sym", "k", "M", "S", "V", "stream"]
    ok = dict(logits=ONE, logits_f32=0, ld=512, out=ONE, fed_ids=ONE, active=ONE, counts=ONE, ctx=ONE, stat=ONE, levels=ONE, end_num=ONE,
              end_min_tokens=8, count=ONE, length=ONE, finish=ONE, alphabet=alpha.data_ptr(), n_sym=4, k=3, M=64, S=4, V=512, stream=None)
    assert list(ok) == names and len(evo_ops._SIGNATURES[NAME][0]) == len(names)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return f(*[a[n] for n in names])
    for n in ("logits", "out", "active", "counts", "ctx", "stat", "levels", "alphabet"):
        assert call(**{n: None}) == -1, n
    for n in ("logits", "out"):                                       # 16-byte alignment
        assert call(**{n: ctypes.c_void_p(8)}) == -1 and call(**{n: ctypes.c_void_p(24)}) == -1, n
    for n in ("counts", "ctx", "levels", "end_num"):                 # their element's alignment
        assert call(**{n: ctypes.c_void_p(18)}) == -1, n
    for n in ("stat", "fed_ids", "count", "length"):
        assert call(**{n: ctypes.c_void_p(20)}) == -1, n
    for n_sym in (0, 9, -1):
        assert call(n_sym=n_sym) == -1, n_sym
    for ids in ([A, C, G, 512], [A, C, G, -1], [A, C, G, A], [A, A, G, T], [1 << 20, C, G, T]):
        bad = torch.tensor(ids, dtype=torch.int32)
        assert call(alphabet=bad.data_ptr()) == -1, ids
    eight = torch.tensor([0, 7, 8, 504, 511, 65, 66, 65], dtype=torch.int32)            # a duplicate in the last of 8 places
    assert call(alphabet=eight.data_ptr(), n_sym=8, k=1, M=8) == -1
    for k in (0, -1, 1 << 31):
        assert call(k=k) == -1, k
    for kw in (dict(M=63), dict(M=65), dict(M=0), dict(k=2), dict(k=4), dict(k=11, M=4 ** 11), dict(k=21, M=64), dict(k=40, M=64),
               dict(n_sym=1, k=5, M=2), dict(n_sym=1, k=5, M=5)):
        assert call(**kw) == -1, kw
    assert call(V=256) == -1 and call(S=0) == -1 and call(S=-3) == -1 and call(ld=500) == -1 and call(ld=516) == -1
    for n in ("count", "length", "finish"):                          # the early end needs where to say so
        assert call(**{n: None}) == -1, n
    assert call(end_min_tokens=0) == -1


# ------------------------------------------------------------------------------------------------ the written rule
def _fold_all(ids, k, tokens, generated=False):
    st = RepeatState(ids, k)
    for t in tokens:
        H.repeat_fold(st, t, generated)
    return st


def test_fold_counts_kmers_at_k_1_2_3():
    text = [ord(c) for c in "ACGACGA"]
    st = _fold_all(ACGT, 1, text)                                     # k = 1: a per-token count, the window is always empty
    assert st.counts.tolist() == [3, 2, 2, 0] and (st.code, st.len) == (0, 0) and (st.n_gen, st.rep) == (0, 0)
    st = _fold_all(ACGT, 2, text)
    want = [0] * 16
    want[0 * 4 + 1], want[1 * 4 + 2], want[2 * 4 + 0] = 2, 2, 2       # AC, CG, GA
    assert st.counts.tolist() == want and (st.code, st.len) == (0, 1)    # the window: A
    st = _fold_all(ACGT, 3, text)
    want = [0] * 64
    want[(0 * 4 + 1) * 4 + 2], want[(1 * 4 + 2) * 4 + 0], want[(2 * 4 + 0) * 4 + 1] = 2, 2, 1      # ACG x 2, CGA x 2, GAC
    assert st.counts.tolist() == want and (st.code, st.len) == (2 * 4 + 0, 2)                   # the window: GA, newest in the lowest digit
    # generated tokens: every one counts in n_gen, one that completes a k-mer seen before in rep
    gen = _fold_all(ACGT, 3, text, generated=True)
    assert (gen.n_gen, gen.rep) == (7, 2) and torch.equal(gen.counts, st.counts)          # the second ACG and the second CGA


def test_a_token_outside_the_alphabet_empties_the_window():
    N = ord("N")
    st = _fold_all(ACGT, 3, [A, C, N, G, A])
    assert int(st.counts.sum()) == 0 and (st.code, st.len) == (2 * 4 + 0, 2)            # ACN, CNG, NGA are no 3-mers
    H.repeat_fold(st, C, True)
    assert int(st.counts[(2 * 4 + 0) * 4 + 1]) == 1 and (st.n_gen, st.rep) == (1, 0)
    H.repeat_fold(st, N, True)                                        # a generated token outside the alphabet still counts in n_gen
    assert (st.code, st.len) == (0, 0) and (st.n_gen, st.rep) == (2, 0)
    H.repeat_fold(st, 0, True)                                        # (a BOS-like id)
    assert (st.code, st.len, st.n_gen) == (0, 0, 3)


def test_penalise_touches_symbols_only_and_only_with_a_full_window():
    lv = torch.tensor([0, 1, 2, 3, 4, 5, 6, 7.5], dtype=torch.float32)
    row = torch.arange(512, dtype=torch.float32) * 0.25 - 17.0
    st = _fold_all(ACGT, 3, [A])                                      # len = 1 < k - 1: unchanged
    assert torch.equal(H.repeat_penalise(row, st, lv), row)
    st = _fold_all(ACGT, 3, [A, C])                                   # window AC, nothing seen: levels[0] == 0 leaves every bit
    assert torch.equal(H.repeat_penalise(row, st, lv), row)
    base = (0 * 4 + 1) * 4
    st.counts[base + 0], st.counts[base + 1], st.counts[base + 2], st.counts[base + 3] = 1, 6, 7, 8
    out = H.repeat_penalise(row, st, lv)
    want = row.clone()
    for t, v in zip(ACGT, (1.0, 6.0, 7.5, 7.5)):                      # a count of 7 and of 8 take the last level
        want[t] = row[t] - torch.tensor(v, dtype=torch.float32)
    assert torch.equal(out, want) and not torch.equal(out, row) and out is not row
    st.counts[base + 3] = 2 ** 31 - 1
    assert torch.equal(H.repeat_penalise(row, st, lv), want)
    # k = 1: the window is always full
    st = _fold_all(ACGT, 1, [G, G, T])
    out = H.repeat_penalise(row, st, lv)
    assert float(out[G]) == float(row[G]) - 2.0 and float(out[T]) == float(row[T]) - 1.0 and float(out[A]) == float(row[A])
    with pytest.raises(ValueError):
        H.repeat_penalise(row.double(), st, lv)


def test_counts_saturate():
    st = _fold_all(ACGT, 2, [A])
    st.counts[0] = 2 ** 31 - 2
    H.repeat_fold(st, A, True)
    assert int(st.counts[0]) == 2 ** 31 - 1 and st.rep == 1
    H.repeat_fold(st, A, True)
    assert int(st.counts[0]) == 2 ** 31 - 1 and st.rep == 2           # saturated, still a repeat


def test_a_window_outside_its_invariants_reads_as_empty():
    for code, ln in ((16, 2), (-1, 2), (3, 3), (3, -1)):
        st = RepeatState(ACGT, 3, code=code, length=ln)
        assert st.window() == (0, 0)
        H.repeat_fold(st, C, True)
        assert (st.code, st.len) == (1, 1) and int(st.counts.sum()) == 0


def test_repeat_init_with_and_without_the_prompt():
    prompt = [0] + [ord(c) for c in "ACGACG"]                         # a BOS in front
    on = H.repeat_init(prompt, SimpleNamespace(ids=ACGT, k=3, count_prompt=True))
    off = H.repeat_init(prompt, SimpleNamespace(ids=ACGT, k=3, count_prompt=False))
    assert int(on.counts.sum()) == 4 and int(off.counts.sum()) == 0
    assert (on.code, on.len) == (off.code, off.len) == (1 * 4 + 2, 2) and (on.n_gen, on.rep, off.n_gen, off.rep) == (0, 0, 0, 0)
    H.repeat_fold(on, A, True)                                        # CGA: seen in the prompt
    H.repeat_fold(off, A, True)                                       # completes a 3-mer with the prompt's tail, never counted before
    assert (on.rep, off.rep) == (1, 0) and int(off.counts[(1 * 4 + 2) * 4 + 0]) == 1


def test_the_end_rule_on_its_boundaries():
    st = RepeatState(ACGT, 2)
    st.n_gen, st.rep = 64, 16                                         # rep * 1024 == 256 * n_gen: exactly a quarter
    assert not H.repeat_ended(st, 256, 8)
    st.rep = 17
    assert H.repeat_ended(st, 256, 8)
    assert not H.repeat_ended(st, 0, 8) and not H.repeat_ended(st, -5, 8)      # not armed
    st.n_gen, st.rep = 7, 7
    assert not H.repeat_ended(st, 256, 8)                             # n_gen == end_min_tokens - 1
    st.n_gen = 8
    assert H.repeat_ended(st, 256, 8)                                 # n_gen == end_min_tokens
    st.n_gen, st.rep = 2 ** 40, 2 ** 38 + 1                           # integers all the way
    assert H.repeat_ended(st, 256, 8) and not H.repeat_ended(st, 257, 8)


def test_repeat_control_resolves():
    r = RepeatControl().resolve(TOK, None)
    assert (r.k, r.ids, r.M, r.end_num, r.end_min_tokens, r.count_prompt) == (8, ACGT, 4 ** 8, 0, 64, True)
    assert r.levels.dtype == torch.float32 and r.levels.tolist() == [0.0, 1.0, 2.0, 3.0, 4.0, 4.0, 4.0, 4.0]
    r = RepeatControl(k=2, penalty=0.3, max_count=2, end_fraction=0.25, end_min_tokens=8).resolve(TOK, H.allowed_mask(TOK, "ACGTN"))
    assert r.ids == tuple(sorted(ord(c) for c in "ACGTN")) and r.M == 25 and r.end_num == 256
    f32 = lambda v: float(torch.tensor(v, dtype=torch.float64).to(torch.float32))
    assert r.levels.tolist() == [0.0, f32(0.3), f32(0.6)] + [f32(0.6)] * 5
    r = RepeatControl(k=1, levels=[0, 2.5], alphabet="AT").resolve(TOK, None)
    assert r.ids == (A, T) and r.levels.tolist() == [0.0] + [2.5] * 7
    assert RepeatControl(k=5, alphabet=[7]).resolve(None, None).M == 1


# ------------------------------------------------------------------------------------------------ the pool on the oracle backend
class RepeatOracleOps(PagedCtlOps):
    """The oracle backend + the repeat launch, row by row from the written specification."""
    repeat_calls = 0

    def repeat_rows(self, logits, out, active, counts, ctx, stat, levels, alphabet, k, fed_ids=None, end_num=None, end_min_tokens=1,
                    count=None, length=None, finish=None):
        type(self).repeat_calls += 1
        for s in range(logits.shape[0]):
            if not bool(active[s]):
                continue
            st = RepeatState(alphabet.tolist(), k, counts[s], int(ctx[s, 0]), int(ctx[s, 1]), int(stat[s, 0]), int(stat[s, 1]))
            row = H.repeat_row(logits[s], st, levels[s], None if fed_ids is None else int(fed_ids.view(-1)[s]),
                               None if end_num is None else int(end_num[s]), end_min_tokens)
            counts[s] = st.counts
            if fed_ids is not None:
                ctx[s, 0], ctx[s, 1], stat[s, 0], stat[s, 1] = st.code, st.len, st.n_gen, st.rep
            if row is None:
                active[s], length[s], finish[s] = False, int(count[s]), H.FINISH_REPEAT
            else:
                out[s] = row
        return out


@pytest.fixture(scope="module")
def small():
    return _model(RepeatOracleOps(torch.float64))


SEED, TOP_K, TEMP, N_SPP, N_TOK = 11, 4, 10.0, 2, 24
N_JOBS = len(PROMPTS) * N_SPP


def run(m, repeat, n_tokens=N_TOK, **kw):
    gen = {k: kw.pop(k) for k in ("stop_sequences", "constraints", "return_logits") if k in kw}
    pool = DecodePool(m, TOK, n_slots=3, top_k=TOP_K, top_p=1.0, temperature=TEMP, device="cpu", seed=SEED, allowed_tokens="ACGT", **kw)
    if repeat is not None:
        gen["repeat"] = repeat
    out = pool.generate(PROMPTS, n_tokens=n_tokens, n_sample_per_prompt=N_SPP, **gen)
    return (pool,) + tuple(out)


def replay(prompt, ids, r, limit, by_rule):
    """The rule on one job's tokens, launch by launch -> (length, finish or 0, (n_gen, rep) as the device holds them at that point).
    `by_rule`: the job's finish was "repeat" -- one more launch ran after its last token; otherwise the sampler ended it with that token."""
    st = H.repeat_init([ord(c) for c in prompt], r)
    n = 0
    while True:
        if n == len(ids) and not by_rule:
            return n, 0, (st.n_gen, st.rep)
        if n:
            H.repeat_fold(st, ids[n - 1], True)
        if r.end_num and H.repeat_ended(st, r.end_num, r.end_min_tokens):
            return n, H.FINISH_REPEAT, (st.n_gen, st.rep)
        if n == len(ids):
            return n, 0, (st.n_gen, st.rep)
        n += 1
        if n >= limit:
            return n, H.FINISH_LENGTH, (st.n_gen, st.rep)


def check_against_replay(pool, owner, r, limit=N_TOK):
    ends = 0
    for j in range(len(owner)):
        n = pool.last_lengths[j]
        ids = pool.last_ids[j, :n].tolist()
        fin = {v: k for k, v in H.FINISH_NAMES_REPEAT.items()}[pool.last_finish[j]]
        got = replay(PROMPTS[owner[j]], ids, r, limit, fin == H.FINISH_REPEAT)
        if fin in (H.FINISH_REPEAT, H.FINISH_LENGTH):
            assert got[:2] == (n, fin), (j, got, n, fin)
        else:                                                         # another rule ended it sooner: the repeat rule had not fired
            assert got[:2] == (n, 0), (j, got, n, fin)
        assert pool.last_repeats[j] == got[2], (j, pool.last_repeats[j], got)
        assert got[2][0] == (n if fin == H.FINISH_REPEAT else n - 1)  # a job the sampler ended has its last token unfolded
        assert bool((pool.last_ids[j, n:] == -1).all())
        ends += fin == H.FINISH_REPEAT
    assert pool.stats["repeat_ends"] == ends
    return ends


def test_zero_levels_change_nothing_and_the_statistics_equal_a_recount(small):
    base = run(small, None, n_tokens=[N_TOK] * len(PROMPTS))         # the job-control path without the launch
    calls = RepeatOracleOps.repeat_calls
    rc = RepeatControl(k=3, penalty=0.0)
    pool, seqs, scores, owner = run(small, rc)
    assert RepeatOracleOps.repeat_calls > calls
    assert torch.equal(pool.last_ids, base[0].last_ids) and torch.equal(pool.last_logits, base[0].last_logits)
    assert pool.last_lengths == base[0].last_lengths == [N_TOK] * N_JOBS and pool.last_finish == base[0].last_finish == ["length"] * N_JOBS
    assert seqs == base[1] and owner == base[3]
    assert not hasattr(base[0], "last_repeats") and "repeat_ends" not in base[0].stats and pool.stats["repeat_ends"] == 0
    assert check_against_replay(pool, owner, rc.resolve(TOK, pool.allow_mask)) == 0
    assert any(rep > 0 for _, rep in pool.last_repeats)               # (the prompts repeat themselves: some 3-mers come again)
    # without the prompt's k-mers the counts start empty, the window does not
    off = RepeatControl(k=3, penalty=0.0, count_prompt=False)
    p2, _, _, owner2 = run(small, off)
    assert torch.equal(p2.last_ids, pool.last_ids)
    check_against_replay(p2, owner2, off.resolve(TOK, p2.allow_mask))
    assert sum(rep for _, rep in p2.last_repeats) < sum(rep for _, rep in pool.last_repeats)
    # the same pool without `repeat` again: the launch is gone, and so is what described the earlier run
    calls = RepeatOracleOps.repeat_calls
    pool.generate(PROMPTS, n_tokens=[N_TOK] * len(PROMPTS), n_sample_per_prompt=N_SPP)
    assert RepeatOracleOps.repeat_calls == calls and not hasattr(pool, "last_repeats")
    assert torch.equal(pool.last_ids, base[0].last_ids)


def test_the_pool_init_equals_the_rule(small):
    pool = DecodePool(small, TOK, n_slots=3, device="cpu", seed=1)
    N = ord("N")
    for k, ids, on in ((1, ACGT, True), (2, ACGT, True), (3, ACGT, False), (8, ACGT, True), (5, (A,), True), (6, (A, C, G, T, N), True)):
        r = SimpleNamespace(ids=ids, n_sym=len(ids), k=k, M=H.repeat_table_size(len(ids), k), count_prompt=on)
        for text in PROMPTS + ["ACNNGTACGTNACGTACGTACGTAAAAAAAAAAAAAAN", "NACGTACGTA", "A"]:
            toks = [0] + [ord(c) for c in text]
            want = H.repeat_init(toks, r)
            counts, ctx = pool._repeat_init(torch.tensor(toks), r)
            assert counts.dtype == torch.int32 and torch.equal(counts, want.counts) and ctx.tolist() == [want.code, want.len], (k, ids, text)


def test_jobs_end_where_the_rule_ends_them_and_their_slots_are_refilled(small):
    rc = RepeatControl(k=2, penalty=0.0, end_fraction=0.25, end_min_tokens=8)
    pool, seqs, scores, owner = run(small, rc)
    ends = check_against_replay(pool, owner, rc.resolve(TOK, pool.allow_mask))
    assert ends >= 1 and "repeat" in pool.last_finish and len(seqs) == N_JOBS > 3       # every job ran: freed slots were refilled
    for j in range(N_JOBS):
        if pool.last_finish[j] == "repeat":                           # a job the rule ended keeps all its tokens
            assert 8 <= pool.last_lengths[j] < N_TOK and len(seqs[j]) == pool.last_lengths[j]
    assert pool.stats["repeat_ends"] + pool.stats["length_ends"] == N_JOBS and pool.stats["polls"] > 0
    assert not bool(pool.s_active.any())
    # poll_every changes the number of reads, nothing else
    p1, s1, _, _ = run(small, rc, poll_every=1)
    assert s1 == seqs and p1.last_finish == pool.last_finish and p1.last_repeats == pool.last_repeats and torch.equal(p1.last_ids, pool.last_ids)


def test_a_huge_level_forbids_every_seen_kmer_that_has_an_alternative(small):
    rc = RepeatControl(k=3, levels=[0, 1e30])
    pool, seqs, _, owner = run(small, rc)
    r = rc.resolve(TOK, pool.allow_mask)
    forced = free = 0
    for j in range(N_JOBS):
        st = H.repeat_init([ord(c) for c in PROMPTS[owner[j]]], r)
        for t in pool.last_ids[j, :pool.last_lengths[j]].tolist():
            code, ln = st.window()
            if ln == 2:
                seen = [int(st.counts[code * 4 + a]) >= 1 for a in range(4)]
                if seen[ACGT.index(t)]:
                    assert all(seen), (j, seqs[j])
                    forced += 1
                else:
                    free += 1
            H.repeat_fold(st, t, True)
    assert free > 0
    print(f"[repeat forbid] {free} draws of an unseen 3-mer, {forced} where all four were seen")
    # the recorded logits are the rows the sampler drew from: the penalised ones
    assert bool((pool.last_logits[:, :, list(ACGT)] < -1e29).any())


def test_with_a_stop_sequence_and_a_constraint(small):
    tpl = K.iupac_template("ACGTNNNNNNNNNNNNNNNN")
    rc = RepeatControl(k=2, penalty=0.5, end_fraction=0.5, end_min_tokens=6)
    cons = [tpl, None, None, tpl, None, None]
    pool, seqs, _, owner = run(small, rc, stop_sequences=["TA", "GG"], constraints=cons)
    check_against_replay(pool, owner, rc.resolve(TOK, pool.allow_mask))
    for j, s in enumerate(seqs):
        if cons[owner[j]] is not None:
            assert s.startswith("ACGT"[:len(s)]), s
        if pool.last_finish[j] == "stop_sequence":
            assert s.endswith(("TA", "GG"))
    assert set(pool.last_finish) <= {"stop_sequence", "constraint", "length", "repeat"} and len(set(pool.last_finish)) >= 2
    assert sum(pool.stats[k] for k in ("stop_ends", "constraint_ends", "length_ends", "repeat_ends")) == N_JOBS


def test_composes_with_the_pool_options(small):
    rc = RepeatControl(k=2, penalty=0.25, end_fraction=0.25, end_min_tokens=8)
    want = run(small, rc)
    for kw in (dict(share_prompt_kv=True), dict(kv_paged=True, kv_page_tokens=64), dict(return_logits=False)):
        pool, seqs, scores, owner = run(small, rc, **kw)
        assert torch.equal(pool.last_ids, want[0].last_ids) and pool.last_finish == want[0].last_finish, kw
        assert pool.last_repeats == want[0].last_repeats and seqs == want[1], kw
    _, sm_seqs, _ = sample_many(PROMPTS, small, TOK, n_tokens=N_TOK, temp=TEMP, top_k=TOP_K, n_sample_per_prompt=N_SPP, n_slots=3, device="cpu",
                                seed=SEED, allowed_tokens="ACGT", repeat=rc)
    assert sm_seqs == want[1]


# ------------------------------------------------------------------------------------------------ refusals
def test_what_is_refused_before_any_forward(small):
    mk = lambda **kw: DecodePool(small, TOK, n_slots=2, device="cpu", seed=1, **kw)
    bad = [dict(k=0), dict(k=-2), dict(k=11), dict(k=2.5), dict(alphabet=""), dict(alphabet="ACGTNRYKM"), dict(alphabet="AACG"),
           dict(alphabet=[A, 300]), dict(alphabet=[A, -1]), dict(levels=[1.0, 2.0]), dict(levels=[]), dict(levels=[0.0] * 9),
           dict(levels=[0, float("inf")]), dict(levels=[0, float("nan")]), dict(levels=[0, 1e39]), dict(penalty=float("inf")),
           dict(end_fraction=0.0), dict(end_fraction=1.0), dict(end_fraction=-0.25), dict(end_fraction=1.5), dict(end_fraction=float("nan")),
           dict(end_fraction=1e-5), dict(end_fraction=0.9999), dict(end_min_tokens=0), dict(max_count=-1)]
    steps = RepeatOracleOps.repeat_calls
    for kw in bad:
        pool = mk()
        with pytest.raises(ValueError, match="repeat"):
            pool.generate(PROMPTS[:1], n_tokens=4, repeat=RepeatControl(**kw))
        assert pool.stats["prefills"] == 0 and pool.ipd is None, kw
    pool = mk(allowed_tokens="ACG")
    with pytest.raises(ValueError, match="allowed_tokens"):
        pool.generate(PROMPTS[:1], n_tokens=4, repeat=RepeatControl(alphabet="ACGT"))
    with pytest.raises(ValueError, match="RepeatControl"):
        mk().generate(PROMPTS[:1], n_tokens=4, repeat={"k": 3})
    assert mk(allowed_tokens="ACG").generate(PROMPTS[:1], n_tokens=3, repeat=RepeatControl(k=2))[0][0]      # None: the pool's allowed tokens
    plain = mk()
    plain.model = SimpleNamespace(ops=SimpleNamespace(sample_rows_ctl=None), device=torch.device("cpu"))      # a backend without the launch
    with pytest.raises(RuntimeError, match="repeat_rows"):
        plain.generate(PROMPTS[:1], n_tokens=4, repeat=RepeatControl())
    assert RepeatOracleOps.repeat_calls > steps                       # (only the one run that was allowed)


def test_the_cli_builds_one_control(tmp_path, monkeypatch):
    """Every flag lands in ONE RepeatControl handed to DecodePool.generate (a recording pool stands in: no model is loaded)."""
    import evo_amd.pool
    import scripts.sample_many as cli
    calls = []

    class RecordingPool:
        stats = {"steps": 0, "prefills": 0}
        last_lengths, last_finish, last_repeats = [5, 3], ["length", "repeat"], [(4, 1), (3, 2)]

        def __init__(self, *a, **kw):
            pass

        def generate(self, prompts, **kw):
            calls.append((list(prompts), kw))
            return ["ACGTA", "GGG"], [-1.0, -2.0], [0, 1]
    monkeypatch.setattr(evo_amd, "Evo", lambda *a, **kw: SimpleNamespace(model=None, tokenizer=None))
    monkeypatch.setattr(evo_amd.pool, "DecodePool", RecordingPool)
    (tmp_path / "p.txt").write_text("ACGT\nGG\n")
    base = ["--prompts", str(tmp_path / "p.txt"), "--output-csv", str(tmp_path / "out.csv"), "--n-tokens", "30"]
    header = lambda: (tmp_path / "out.csv").read_text().splitlines()[0].split(",")
    cli.main(base + ["--extra-columns"])
    assert "repeat" not in calls[-1][1] and header()[-2:] == ["Length", "Finish"]       # without the flags the call and the file are what they were
    rows = cli.main(base + ["--repeat-k", "6", "--extra-columns"])
    rc = calls[-1][1]["repeat"]
    assert isinstance(rc, RepeatControl) and (rc.k, rc.penalty, rc.max_count, rc.count_prompt, rc.end_fraction, rc.end_min_tokens) \
        == (6, 1.0, 4, True, None, 64)
    assert header()[-3:] == ["Length", "Finish", "Repeats"] and [r[-3:] for r in rows] == [["5", "length", "1"], ["3", "repeat", "2"]]
    cli.main(base + ["--repeat-k", "3", "--repeat-penalty", "0.5", "--repeat-max-count", "2", "--repeat-ignore-prompt", "--repeat-end-fraction",
                     "0.4", "--repeat-end-min-tokens", "16"])
    rc = calls[-1][1]["repeat"]
    assert (rc.k, rc.penalty, rc.max_count, rc.count_prompt, rc.end_fraction, rc.end_min_tokens) == (3, 0.5, 2, False, 0.4, 16)
    assert header()[-1] == "Score"                                    # no --extra-columns: no new column either
    n = len(calls)
    for flags in (["--repeat-penalty", "0.5"], ["--repeat-end-fraction", "0.4"], ["--repeat-ignore-prompt"], ["--repeat-max-count", "2"],
                  ["--repeat-end-min-tokens", "9"]):
        with pytest.raises(SystemExit):                               # they apply with --repeat-k only
            cli.main(base + flags)
    assert len(calls) == n
