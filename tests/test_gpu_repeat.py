"""GPU (-m gpu): k-mer repeat control of the decode pool -- the kernel `evo_repeat_rows_f32` (csrc/repeat.hip,
HipOps.repeat_rows) against the written rule (evo_amd/sh/sample.py: repeat_row), and the pool that runs on it.

  * kernel: chains of 12 launches; `out`, `counts`, `ctx`, `stat`, `active`, `length` and `finish` equal the specification bit for bit after
    every launch.  Each launch feeds the specification's own seeded draw from the previous row (and now and then a token outside the
    alphabet), so the state carries.  `out` is poisoned with 0xFF before every launch: inactive rows and the rows of ended jobs keep it.
    The same chain run again from the same state gives the same bits;
  * arena: the entry inside a poisoned arena (`covers()` registers it at import time for tests/test_gpu_arena.py's
    test_every_entry_point_is_named_by_a_case);
  * pool: on the toy model, 4 slots, at most 32 tokens, captured and eager."""
import gc
from types import SimpleNamespace

import pytest
import torch

import evo_amd.ops as evo_ops
from evo_amd import constraints as K
from evo_amd.sh import sample as H
from evo_amd.sh.sample import RepeatControl, RepeatState
from test_gpu_arena import _run, covers, gen, is_poison, poisoned, rnd
from test_gpu_model import DEV
from test_gpu_pool import PROMPTS
from test_repeat_host import check_against_replay

pytestmark = pytest.mark.gpu
A, C, G, T = (ord(c) for c in "ACGT")
ACGT = (A, C, G, T)
L = 12
SEED = 4242
OUTSIDE = 3                                                           # a token of no alphabet below
ALPHABETS = {1: [511], 2: [0, 7], 4: [A, C, G, T], 8: [0, 7, 8, 504, 511, 65, 71, 300]}      # lane 0 twice, lane 63 twice, lane edges
PRESET = [0, 1, 6, 7, 8, 2 ** 31 - 1]
END_MIN = 4
STATS = [(64, 16), (64, 17), (2, 2), (0, 0)]                          # at end_num = 256: on the boundary, past it, too young, fresh


def ops():
    return evo_ops.default_ops()


def bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


class Chain:
    """The CPU state of one chain (one RepeatState per row and the per-row vectors) and what is needed to put a copy on the device."""

    def __init__(self, S, n_sym, k, f32, ld, end):
        g = torch.Generator().manual_seed(1000 * S + 37 * n_sym + k)
        self.S, self.k, self.ids, self.end = S, k, ALPHABETS[n_sym], end
        self.M = H.repeat_table_size(n_sym, k)
        self.alpha = torch.tensor(self.ids, dtype=torch.int32)
        self.allowed = H.allowed_mask(None, self.ids)
        rows = torch.randn(L, S, ld, generator=g) * 3.0
        self.rows_cpu = rows if f32 else rows.bfloat16()
        self.ld = ld
        self.states, self.active = [], torch.ones(S, dtype=torch.bool)
        for s in range(S):
            ln = (k - 1) // 2 if (S > 1 and k > 1 and s % 3 == 0) else k - 1     # some rows start with a short window
            code = int(torch.randint(0, n_sym ** ln, (1,), generator=g)) if n_sym > 1 else 0
            n_gen, rep = STATS[s % 4]
            st = RepeatState(self.ids, k, None, code, ln, n_gen, rep)
            for _ in range(min(self.M, 48)):                          # a sprinkle of small counts ...
                st.counts[int(torch.randint(0, self.M, (1,), generator=g))] = int(torch.randint(1, 4, (1,), generator=g))
            if ln == k - 1:                                           # ... and the cells the first launch reads: 0, 1, 6, 7, 8, 2^31 - 1
                for a in range(n_sym):
                    st.counts[code * n_sym + a] = PRESET[(s + a) % len(PRESET)]
            self.states.append(st)
            if S > 2 and s % 5 == 2:
                self.active[s] = False
        lv = (torch.randn(S, 8, generator=g) * 2.0).abs().float()
        lv[:, 0] = 0.0
        self.levels = lv
        self.end_num = torch.tensor([0 if s % 3 == 0 and S > 1 else 256 for s in range(S)], dtype=torch.int32)
        self.count = torch.arange(S, dtype=torch.int64) + 5

    def device_state(self):
        st = self.states
        return dict(counts=torch.stack([x.counts for x in st]).to(DEV), ctx=torch.tensor([[x.code, x.len] for x in st], dtype=torch.int32, device=DEV),
                    stat=torch.tensor([[x.n_gen, x.rep] for x in st], dtype=torch.int64, device=DEV), active=self.active.clone().to(DEV),
                    length=poisoned((self.S,), torch.int64), finish=poisoned((self.S,), torch.uint8), out=poisoned((self.S, 512), torch.float32))

    def launch(self, dev, t, fed):
        dev["out"].view(-1).view(torch.uint8).fill_(0xFF)
        end = dict(end_num=self.end_dev, end_min_tokens=END_MIN, count=self.count_dev, length=dev["length"], finish=dev["finish"]) if self.end else {}
        ops().repeat_rows(self.rows_dev[t][:, :512], dev["out"], dev["active"], dev["counts"], dev["ctx"], dev["stat"], self.levels_dev, self.alpha,
                          self.k, fed_ids=None if fed is None else fed.to(DEV), **end)

    def run(self):
        """L launches checked against the rule after each one; then the same launches again from the same starting state."""
        S = self.S
        self.rows_dev, self.levels_dev = self.rows_cpu.to(DEV), self.levels.to(DEV)
        self.end_dev, self.count_dev = self.end_num.to(DEV), self.count.to(DEV)
        first, again = self.device_state(), self.device_state()
        want_len, want_fin = first["length"].cpu(), first["finish"].cpu()
        fed, feds, seen = None, [], set()
        for t in range(L):
            want_out = poisoned((S, 512), torch.float32).cpu()
            for s in range(S):
                if not bool(self.active[s]):
                    continue
                st = self.states[s]
                row = H.repeat_row(self.rows_cpu[t, s, :512].float(), st, self.levels[s], None if fed is None else int(fed[s]),
                                   int(self.end_num[s]) if self.end else None, END_MIN)
                if row is None:
                    self.active[s], want_len[s], want_fin[s] = False, self.count[s], H.FINISH_REPEAT
                    seen.add("ended")
                else:
                    want_out[s] = row
                    seen.add("full" if st.window()[1] == self.k - 1 else "short")
            self.launch(first, t, fed)
            feds.append(fed)
            got = {k: v.cpu() for k, v in first.items()}
            assert torch.equal(bits(got["out"]), bits(want_out)), (t, torch.nonzero(bits(got["out"]) != bits(want_out))[:4].tolist())
            assert torch.equal(got["counts"], torch.stack([x.counts for x in self.states])), t
            assert got["ctx"].tolist() == [[x.code, x.len] for x in self.states], t
            assert got["stat"].tolist() == [[x.n_gen, x.rep] for x in self.states], t
            assert torch.equal(got["active"], self.active) and torch.equal(got["length"], want_len) and torch.equal(got["finish"], want_fin), t
            # the next launch is fed the rule's own draw from this row; now and then a token outside the alphabet
            fed = torch.full((S,), OUTSIDE, dtype=torch.int64)
            for s in range(S):
                if bool(self.active[s]) and not (t % 5 == 4 and s % 4 == 1):
                    fed[s] = int(H.sample_seeded(want_out[s], 4, 1.0, 1.0, SEED, s, t, self.allowed))
        for t in range(L):
            self.launch(again, t, feds[t])
        torch.cuda.synchronize()
        for k, v in first.items():
            assert torch.equal(bits(v), bits(again[k])), k
        return seen


@pytest.mark.parametrize("n_sym,k", [(4, 1), (4, 2), (4, 3), (4, 8), (1, 5), (2, 7), (8, 6)])
@pytest.mark.parametrize("S", [1, 3, 8])
def test_kernel_equals_the_rule_bit_for_bit(S, n_sym, k):
    seen = set()
    for f32, ld, end in ((False, 512, False), (False, 640, True), (True, 512, True), (True, 640, False)):
        seen |= {(x, end) for x in Chain(S, n_sym, k, f32, ld, end).run()}
    assert ("full", False) in seen and ("full", True) in seen
    if S > 1:
        assert ("ended", True) in seen                                # (row 1 starts past the boundary)
        if k > 1 and n_sym > 1:
            assert ("short", False) in seen
    assert ("ended", False) not in seen


def test_the_boundary_of_the_end_rule_on_the_device():
    """Three rows at rep * 1024 == end_num * n_gen - 0, + 1 repeat, and one token short of end_min_tokens: only the middle one ends."""
    o = ops()
    S, k = 3, 1
    alpha = torch.tensor(ACGT, dtype=torch.int32)
    counts = torch.ones(S, 4, dtype=torch.int32, device=DEV)
    stat = torch.tensor([[63, 15], [63, 16], [2, 2]], dtype=torch.int64, device=DEV)      # after the fold of a seen token: (64, 16), (64, 17), (3, 3)
    state = dict(active=torch.ones(S, dtype=torch.bool, device=DEV), ctx=torch.zeros(S, 2, dtype=torch.int32, device=DEV),
                 length=poisoned((S,), torch.int64), finish=poisoned((S,), torch.uint8), out=poisoned((S, 512), torch.float32))
    lg = rnd((S, 512), gen(1), 3.0)
    o.repeat_rows(lg, state["out"], state["active"], counts, state["ctx"], stat, torch.zeros(S, 8, device=DEV), alpha, k,
                  fed_ids=torch.full((S,), C, dtype=torch.int64, device=DEV), end_num=torch.full((S,), 256, dtype=torch.int32, device=DEV),
                  end_min_tokens=4, count=torch.tensor([9, 8, 7], dtype=torch.int64, device=DEV), length=state["length"], finish=state["finish"])
    torch.cuda.synchronize()
    assert stat.tolist() == [[64, 16], [64, 17], [3, 3]] and state["active"].tolist() == [True, False, True]
    assert int(state["length"][1]) == 8 and int(state["finish"][1]) == 6 and is_poison(state["length"][[0, 2]]) and is_poison(state["finish"][[0, 2]])
    assert is_poison(state["out"][1]) and torch.equal(state["out"][[0, 2]], lg[[0, 2]].float())       # zero levels: the widened rows
    assert counts[:, 1].tolist() == [2, 2, 2]


# ------------------------------------------------------------------------------------------------ arena
@covers("evo_repeat_rows_f32")
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("armed", [False, True], ids=["plain", "armed"])
def test_repeat_rows_in_the_arena(armed, f32):
    """S = 6, k = 3 over ACGT (64 cells a row): a row whose window is the LAST code (its four cells end the row -- for the last row, the
    tensor), a short window, an inactive row, a row the rule ends, a row fed a token outside the alphabet.  Per-row vectors at their element's
    alignment, the rows at 16 bytes; the counts carved last."""
    o, g = ops(), gen(7)
    S, k = 6, 3
    alpha = torch.tensor(ACGT, dtype=torch.int32)
    inp = {"lg": rnd((S, 520), g, 3.0, torch.float32 if f32 else torch.bfloat16), "out": poisoned((S, 512), torch.float32),
           "fed": torch.tensor([A, C, G, T, OUTSIDE, T], dtype=torch.int64, device=DEV),
           "active": torch.tensor([True, True, False, True, True, True], device=DEV),
           "ctx": torch.tensor([[15, 2], [2, 1], [5, 2], [0, 2], [7, 2], [15, 2]], dtype=torch.int32, device=DEV),
           "stat": torch.tensor([[0, 0], [5, 1], [9, 9], [40, 30], [3, 0], [11, 2]], dtype=torch.int64, device=DEV),
           "levels": torch.tensor([[0, 1, 2, 3, 4, 5, 6, 7]] * S, dtype=torch.float32, device=DEV),
           "end_num": torch.full((S,), 512, dtype=torch.int32, device=DEV), "count": torch.arange(S, dtype=torch.int64, device=DEV) + 20,
           "length": poisoned((S,), torch.int64), "finish": poisoned((S,), torch.uint8),
           "counts": torch.randint(0, 9, (S, 64), generator=g, device=DEV).to(torch.int32)}

    def fn(lg, out, fed, active, ctx, stat, levels, end_num, count, length, finish, counts):
        end = dict(end_num=end_num, end_min_tokens=8, count=count, length=length, finish=finish) if armed else {}
        o.repeat_rows(lg[:, :512], out, active, counts, ctx, stat, levels, alpha, k, fed_ids=fed, **end)
    before = {n: inp[n].clone() for n in ("counts", "ctx", "stat")}
    run = _run(fn, inp, inout=["out", "active", "counts", "ctx", "stat", "length", "finish"], expect=["evo_repeat_rows_f32"],
               align={"fed": 8, "active": 1, "ctx": 4, "stat": 8, "levels": 4, "end_num": 4, "count": 8, "length": 8, "finish": 1, "counts": 4})
    got = run.inputs
    assert got["active"].tolist() == [True, True, False, not armed, True, True]
    assert is_poison(got["out"][2]) and is_poison(got["out"][3]) == armed and not is_poison(got["out"][0])
    assert torch.equal(got["counts"][2], before["counts"][2]) and got["ctx"][2].tolist() == [5, 2] and got["stat"][2].tolist() == [9, 9]
    assert got["ctx"][0].tolist() == [(15 * 4 + 0) % 16, 2] and got["ctx"][1].tolist() == [2 * 4 + 1, 2] and got["ctx"][4].tolist() == [0, 0]
    assert got["ctx"][5].tolist() == [15, 2] and int(got["counts"][5, 63]) == int(before["counts"][5, 63]) + 1          # the last cell of the tensor
    assert got["stat"][:, 0].tolist() == [1, 6, 9, 41, 4, 12]
    if armed:
        assert int(got["length"][3]) == 23 and int(got["finish"][3]) == 6 and is_poison(got["length"][[0, 1, 2, 4, 5]])
    else:
        assert is_poison(got["length"]) and is_poison(got["finish"])
    assert torch.equal(got["out"][4], inp["lg"][4, :512].float())     # an empty window: the widened row


# ------------------------------------------------------------------------------------------------ pool
N_SPP, N_TOK, POOL_SEED = 2, 32, 5
N_JOBS = len(PROMPTS) * N_SPP
_RUNS = {}


@pytest.fixture(scope="module")
def toy():
    from evo_amd.tokenizer import CharLevelTokenizer
    from test_gpu_paged_kv import _build_toy
    return _build_toy(), CharLevelTokenizer(512)


def run(toy, name, repeat, use_graph=True, n_tokens=N_TOK, n_spp=N_SPP, temperature=1.0, **kw):
    """One pool run: 4 slots, ACGT only, seeded.  Its results are cached by name; the pool and its graph are dropped."""
    if name not in _RUNS:
        from evo_amd.pool import DecodePool
        gen_kw = {k: kw.pop(k) for k in ("constraints",) if k in kw}
        pool = DecodePool(toy[0], toy[1], n_slots=4, top_k=4, top_p=1.0, temperature=temperature, device=DEV, use_graph=use_graph, seed=POOL_SEED,
                          allowed_tokens="ACGT", **kw)
        if repeat is not None:
            gen_kw["repeat"] = repeat
        seqs, scores, owner = pool.generate(PROMPTS, n_tokens=n_tokens, n_sample_per_prompt=n_spp, **gen_kw)
        _RUNS[name] = SimpleNamespace(seqs=seqs, scores=scores, owner=owner, last_ids=pool.last_ids, last_logits=pool.last_logits,
                                      last_logprobs=pool.last_logprobs, last_lengths=pool.last_lengths, last_finish=pool.last_finish,
                                      last_repeats=getattr(pool, "last_repeats", None), stats=dict(pool.stats), allow_mask=pool.allow_mask,
                                      captured=pool._graph is not None, idle=not bool(pool.s_active.any()))
        del pool
        gc.collect()
    return _RUNS[name]


def same(p, q):
    return (torch.equal(p.last_ids, q.last_ids) and torch.equal(p.last_logprobs, q.last_logprobs) and torch.equal(p.last_logits, q.last_logits)
            and p.last_lengths == q.last_lengths and p.last_finish == q.last_finish and p.seqs == q.seqs and p.scores == q.scores)


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_pool_with_zero_levels_is_the_run_without_repeat(toy, use_graph):
    tag = "graph" if use_graph else "eager"
    U = run(toy, "free " + tag, None, use_graph, n_tokens=[N_TOK] * len(PROMPTS))
    rc = RepeatControl(k=3, penalty=0.0)
    P = run(toy, "zero " + tag, rc, use_graph)
    assert same(P, U) and P.captured == use_graph and P.idle and U.last_repeats is None
    assert P.last_finish == ["length"] * N_JOBS and P.stats["repeat_ends"] == 0 and P.stats["steps"] == U.stats["steps"]
    assert check_against_replay(P, P.owner, rc.resolve(toy[1], P.allow_mask), N_TOK) == 0          # the device's statistics: a host recount
    print(f"[repeat pool {tag}] repeats per job at zero levels: {[r for _, r in P.last_repeats]}")


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_pool_jobs_end_where_the_rule_ends_them(toy, use_graph):
    tag = "graph" if use_graph else "eager"
    # (the toy model's samples at T = 1 are close to homopolymer runs: every job would end at end_min_tokens.  At T = 8, with the prompt's
    # own 2-mers left out, the fraction of repeats climbs at its own pace in every job)
    rc = RepeatControl(k=2, penalty=0.0, count_prompt=False, end_fraction=0.25, end_min_tokens=8)
    P = run(toy, "end " + tag, rc, use_graph, temperature=8.0)
    ends = check_against_replay(P, P.owner, rc.resolve(toy[1], P.allow_mask), N_TOK)
    assert ends >= 1 and P.stats["repeat_ends"] == ends and P.stats["repeat_ends"] + P.stats["length_ends"] == N_JOBS and P.idle
    assert all(len(s) == n for s, n in zip(P.seqs, P.last_lengths))   # a job the rule ended keeps all its tokens
    assert same(P, run(toy, "end graph", rc, True, temperature=8.0))  # captured and eager: the same bits
    print(f"[repeat pool {tag}] {ends} of {N_JOBS} jobs ended by the rule, lengths {P.last_lengths}")


def test_pool_huge_level_forbids_seen_kmers(toy):
    rc = RepeatControl(k=3, levels=[0, 1e30])
    P = run(toy, "forbid", rc, True, temperature=8.0)
    r = rc.resolve(toy[1], P.allow_mask)
    check_against_replay(P, P.owner, r, N_TOK)
    forced = free = 0
    for j in range(N_JOBS):
        st = H.repeat_init([ord(c) for c in PROMPTS[P.owner[j]]], r)
        for t in P.last_ids[j, :P.last_lengths[j]].tolist():
            code, ln = st.window()
            if ln == 2:
                seen = [int(st.counts[code * 4 + a]) >= 1 for a in range(4)]
                if seen[ACGT.index(t)]:
                    assert all(seen), (j, P.seqs[j])
                    forced += 1
                else:
                    free += 1
            H.repeat_fold(st, t, True)
    assert free > 0
    print(f"[repeat pool forbid] {free} draws of an unseen 3-mer, {forced} where all four had been seen")


def test_pool_forced_replay_reproduces_the_penalised_rows_and_the_draws(toy):
    """Pool A runs with `repeat` on the batch-invariant step.  Pool B, without it, is forced through A's tokens by one template per prompt
    and records the model's own rows -- the same bits A's launch read, since a row of the invariant step depends on its job alone.  The rule
    applied to B's rows under the replayed state must give A's recorded rows bit for bit, and its draw on them A's tokens."""
    n_tok = 16
    rc = RepeatControl(k=3, penalty=0.75, max_count=3)
    a = run(toy, "replay A", rc, True, n_tokens=n_tok, n_spp=1, batch_invariant=True)
    assert a.last_lengths == [n_tok] * len(PROMPTS) and all(set(s) <= set("ACGT") for s in a.seqs)
    b = run(toy, "replay B", None, True, n_tokens=n_tok, n_spp=1, batch_invariant=True, constraints=[K.iupac_template(s) for s in a.seqs])
    assert b.seqs == a.seqs and b.last_finish == ["constraint"] * len(PROMPTS)
    r = rc.resolve(toy[1], a.allow_mask)
    changed = 0
    for j, p in enumerate(PROMPTS):
        st = H.repeat_init([ord(c) for c in p], r)
        for t in range(n_tok):
            want = H.repeat_penalise(b.last_logits[j, t], st, r.levels)
            assert torch.equal(bits(want), bits(a.last_logits[j, t])), (j, t)
            changed += not torch.equal(want, b.last_logits[j, t])
            tok = int(H.sample_seeded(want, 4, 1.0, 1.0, POOL_SEED, j, t, a.allow_mask))
            assert tok == int(a.last_ids[j, t]), (j, t)
            H.repeat_fold(st, tok, True)
    assert changed > 0                                                # (the penalty did something)


def test_pool_composition_shared_prompt_kv_and_batched_prefill(toy):
    rc = RepeatControl(k=2, penalty=0.5, end_fraction=0.25, end_min_tokens=8)
    P = run(toy, "composed", rc, True, share_prompt_kv=True, prefill_batch=4)
    ends = check_against_replay(P, P.owner, rc.resolve(toy[1], P.allow_mask), N_TOK)
    assert P.stats["repeat_ends"] == ends and P.idle and P.stats["prefills"] < len(PROMPTS)
    assert same(P, run(toy, "composed again", rc, True, share_prompt_kv=True, prefill_batch=4))
