"""GPU (-m gpu): constrained generation by per-job token automata -- the kernel `evo_sample_rows_dfa_f32`
(csrc/sample.hip, HipOps.sample_rows_dfa) against the written rule (evo_amd/sh/sample.py: sample_dfa), and the pool that runs on it.

  * kernel: 12 consecutive launches over histories of 12 cells.  Tokens, counters, `active`, `length`, `finish`, `dfa_state` and the
    histories equal the specification exactly; token, log-probability and recorded logits are bit-identical to `evo_sample_rows_ctl_f32`
    launched with each row's permitted set as its 64 allow bytes; every cell nobody may write keeps its canary (the expected tensors are
    compared whole); the eager launches equal the same launches captured in one graph.  Random automata over alphabets of 1, 4 and 8
    symbols -- ACGT, and ids on lane edges (0, 7 | 8, 504 | 511: two ids in one lane, the first and the last lane) -- and scripted rows;
  * arena: the entry inside a poisoned arena, the table carved last.  `covers()` registers the entry point at IMPORT time: in a whole-suite
    run this module is what names `evo_sample_rows_dfa_f32` for tests/test_gpu_arena.py's test_every_entry_point_is_named_by_a_case;
  * pool: on the toy model of tests/test_gpu_stop.py, 4 slots, seeded.  The results of a run are cached, its pool (caches, histories, the
    graph of its step) is dropped.  While a pool with a captured step lives, a capture outside inference mode must still work
    (evo_amd/pool.py `_capture`)."""
import gc
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from evo_amd import constraints as K
from evo_amd.sh import sample as H
from test_constraints_host import CODE, STOPS
from test_gpu_arena import _run, covers, gen, is_poison, poisoned, rnd
from test_gpu_model import DEV, SMALL4, build
from test_gpu_pool import PROMPTS
from test_gpu_sample import acgt_mask, ops
from test_gpu_stop import N_SPP, POOL_SEED, SET, WEIGHTS_SEED

pytestmark = pytest.mark.gpu
A, C, G, T = (ord(c) for c in "ACGT")
L = 12
SEED = 777
EDGES = [0, 7, 8, 504, 511, 65, 71, 300]                             # lane 0 twice, lane 1, lane 63 twice, and three in between
ALPHABETS = {"acgt": [A, C, G, T], "edges8": EDGES, "edges4": EDGES[:4], "one": [511]}
STATE_CANARY = -77                                                    # dfa_state of a row the launch must not touch


def _random_table(n_sym, g):
    """Three automata of 13, 14 and 13 states in one table [40, 8]: per entry 60 % a next state, 15 % ACCEPT, 25 % forbidden (-1, or another
    negative value: forbidden all the same); columns >= n_sym hold live-looking values that must be ignored."""
    sizes = [13, 14, 13]
    parts = []
    for n in sizes:
        u = torch.rand(n, 8, generator=g)
        nxt = torch.randint(0, n, (n, 8), generator=g, dtype=torch.int32)
        t = torch.where(u < 0.60, nxt, torch.where(u < 0.75, torch.tensor(-2, dtype=torch.int32), torch.tensor(-1, dtype=torch.int32)))
        t[(u >= 0.95)] = -9
        parts.append(t)
    table = torch.cat(parts)
    table[:, n_sym:] = torch.randint(0, 13, (table.shape[0], 8 - n_sym), generator=g, dtype=torch.int32) if n_sym < 8 else table[:, n_sym:]
    return table.contiguous(), [0, 13, 27]


class Case:
    """The device state of one run of L launches and the specification's copy of it."""

    def __init__(self, S, alphabet, table, base, state, limit, active, count, rows_cpu, allow_bool, stop_bool, patterns, frame):
        o = ops()
        self.S, self.alphabet, self.table, self.rows_cpu, self.frame = S, list(alphabet), table, rows_cpu, frame
        self.allow_bool, self.stop_bool, self.patterns = allow_bool, stop_bool, patterns
        self.limit, self.base = limit, base
        self.rows = rows_cpu.to(DEV)
        self.alpha = torch.tensor(self.alphabet, dtype=torch.int32)
        self.next = table.to(DEV)
        self.allow = None if allow_bool is None else o.pack_allow_mask(allow_bool, DEV)
        self.stop_mask = None if stop_bool is None else o.pack_allow_mask(stop_bool, DEV)
        self.stop_seq = o.pack_stop_sequences(patterns) if patterns else None
        self.prm = (torch.full((S,), 4, dtype=torch.int32, device=DEV), torch.full((S,), 1.0, dtype=torch.float32, device=DEV),
                    torch.full((S,), 1.0, dtype=torch.float32, device=DEV))
        self.stream_cpu = torch.arange(S, dtype=torch.int64) * 3 + 1
        self.stream = self.stream_cpu.to(DEV)
        self.init = dict(count=count, active=active, state=state)
        # the specification's state: canaries wherever nothing may be written
        self.w = dict(count=count.clone(), active=active.clone(), state=state.clone(), length=torch.full((S,), -5, dtype=torch.int64),
                      finish=torch.full((S,), 9, dtype=torch.uint8), ids=torch.full((S,), -7, dtype=torch.int64),
                      lp=torch.full((S,), 123.0), hid=torch.full((S, L), -9, dtype=torch.int64), hlp=torch.full((S, L), 777.0),
                      hlg=torch.full((S, L, 512), 777.0))

    def device_state(self):
        S, i = self.S, self.init
        return dict(count=i["count"].clone().to(DEV), active=i["active"].clone().to(DEV), state=i["state"].clone().to(DEV),
                    length=torch.full((S,), -5, dtype=torch.int64, device=DEV), finish=torch.full((S,), 9, dtype=torch.uint8, device=DEV),
                    ids=torch.full((S,), -7, dtype=torch.int64, device=DEV), lp=torch.full((S,), 123.0, dtype=torch.float32, device=DEV),
                    hid=torch.full((S, L), -9, dtype=torch.int64, device=DEV), hlp=torch.full((S, L), 777.0, dtype=torch.float32, device=DEV),
                    hlg=torch.full((S, L, 512), 777.0, dtype=torch.float32, device=DEV))

    def launch(self, st, t, rows=slice(None)):
        ops().sample_rows_dfa(self.rows[t][rows], *(p[rows] for p in self.prm), SEED, count=st["count"][rows], active=st["active"][rows],
                              limit=self.limit_dev[rows], length=st["length"][rows], finish=st["finish"][rows], dfa_alphabet=self.alpha,
                              dfa_next=self.next, dfa_base=self.base_dev[rows], dfa_state=st["state"][rows], stream=self.stream[rows],
                              allow=self.allow, ids_out=st["ids"][rows], logprob_out=st["lp"][rows], hist_ids=st["hid"][rows],
                              hist_logits=st["hlg"][rows], hist_logprob=st["hlp"][rows], stop_mask=self.stop_mask, stop_seq=self.stop_seq,
                              stop_frame=self.frame)

    def run(self):
        """L launches, each checked against the specification and against the control kernel; then the same launches in one graph.
        -> the final (length, finish, state) per row and the set of (finish, count) pairs seen."""
        o, S, w = ops(), self.S, self.w
        self.limit_dev, self.base_dev = self.limit.to(DEV), self.base.to(DEV)
        st = self.device_state()
        ctl = dict(ids=torch.full((S,), -7, dtype=torch.int64, device=DEV), lp=torch.full((S,), 123.0, dtype=torch.float32, device=DEV),
                   hid=torch.full((S, L), -9, dtype=torch.int64, device=DEV), hlp=torch.full((S, L), 777.0, dtype=torch.float32, device=DEV),
                   hlg=torch.full((S, L, 512), 777.0, dtype=torch.float32, device=DEV))
        seen = set()
        for t in range(L):
            pre_count = w["count"].clone()
            groups = {}                                               # permitted set -> the rows that draw from it in this launch
            for s in torch.nonzero(w["active"]).flatten().tolist():
                cnt, q, b = int(w["count"][s]), int(w["state"][s]), int(self.base[s])
                tok, n, fin, new = H.sample_dfa(self.rows_cpu[t, s].float(), 4, 1.0, 1.0, SEED, int(self.stream_cpu[s]), w["hid"][s, :cnt].tolist(),
                                                int(self.limit[s]), self.table, q, self.alphabet, self.allow_bool, self.stop_bool,
                                                self.patterns, self.frame, hist_len=L, base=b)
                if tok is not None:
                    w["ids"][s], w["hid"][s, cnt], w["count"][s] = tok, tok, n
                    w["hlg"][s, cnt] = self.rows_cpu[t, s].float()
                    if b >= 0:
                        w["state"][s] = new
                    mask = self.allow_bool if b < 0 else H.dfa_allowed(self.table, b + q, self.alphabet, self.allow_bool)
                    key = None if mask is None else tuple(torch.nonzero(mask).flatten().tolist())
                    groups.setdefault(key, (mask, []))[1].append(s)
                if fin:
                    w["active"][s], w["length"][s], w["finish"][s] = False, n, fin
                    seen.add((fin, cnt if tok is not None else "no draw"))
            self.launch(st, t)
            # the control kernel on the same rows and counters, one launch per permitted set, that set as its allow bytes
            for mask, members in groups.values():
                act = torch.zeros(S, dtype=torch.bool)
                act[members] = True
                o.sample_rows_ctl(self.rows[t], *self.prm, SEED, count=pre_count.clone().to(DEV), active=act.to(DEV),
                                  limit=torch.full((S,), 99, dtype=torch.int64, device=DEV), length=torch.zeros(S, dtype=torch.int64, device=DEV),
                                  finish=torch.zeros(S, dtype=torch.uint8, device=DEV), stream=self.stream,
                                  allow=None if mask is None else o.pack_allow_mask(mask, DEV), ids_out=ctl["ids"], logprob_out=ctl["lp"],
                                  hist_ids=ctl["hid"], hist_logits=ctl["hlg"], hist_logprob=ctl["hlp"])
            torch.cuda.synchronize()
            got = {k: v.cpu() for k, v in st.items()}
            assert torch.equal(got["ids"], w["ids"]), (t, torch.nonzero(got["ids"] != w["ids"]).flatten()[:8].tolist())
            assert torch.equal(got["count"], w["count"]) and torch.equal(got["active"], w["active"]), t
            assert torch.equal(got["length"], w["length"]) and torch.equal(got["finish"], w["finish"]), t
            assert torch.equal(got["state"], w["state"]) and torch.equal(got["hid"], w["hid"]), t
            # bit-identical to the control kernel: token and log-probability (rows that do not draw keep their canaries in both)
            assert torch.equal(got["ids"], ctl["ids"].cpu()) and torch.equal(got["lp"], ctl["lp"].cpu()), t
            assert torch.equal(got["hlp"], ctl["hlp"].cpu()), t
        assert torch.equal(got["hlg"], w["hlg"]) and torch.equal(got["hlg"], ctl["hlg"].cpu()) and torch.equal(got["hid"], ctl["hid"].cpu())
        drew = got["hid"] != -9
        assert bool((got["hlp"][~drew] == 777.0).all()) and bool(torch.isfinite(got["hlp"][drew]).all())
        assert not bool(w["active"].any())                            # every job ended within its 12 launches
        # the same 12 launches captured in one graph
        st2 = self.device_state()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for t in range(L):
                self.launch(st2, t)
        g.replay()
        torch.cuda.synchronize()
        for k, v in st.items():
            assert torch.equal(v, st2[k]), k
        self.final = st
        return [(int(w["length"][s]), int(w["finish"][s]), int(w["state"][s])) for s in range(S)], seen


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("alphabet", list(ALPHABETS))
@pytest.mark.parametrize("S", [1, 5, 257])
def test_kernel_on_random_automata_equals_the_rule_and_the_control_kernel(S, alphabet, f32):
    ids = ALPHABETS[alphabet]
    n_sym = len(ids)
    g = torch.Generator().manual_seed(1000 * S + 10 * n_sym + f32)
    table, bases = _random_table(n_sym, g)
    s = torch.arange(S)
    base = torch.tensor([bases[0], bases[1], bases[2], -1], dtype=torch.int64)[s % 4]
    state = torch.randint(0, 13, (S,), generator=g, dtype=torch.int32)
    state[base < 0] = STATE_CANARY
    limit = 1 + (s * 5) % 12
    active = s % 7 != 6
    count = torch.zeros(S, dtype=torch.int64)
    if S > 5:
        state[10], state[14], state[18] = 13, -1, 2 ** 30              # (base 27) one past the table's last row, negative, far past it
        gone = (s % 11 == 10) & (s > 20)
        count[gone] = limit[gone]                                    # active with nothing left to draw: ends by length before the automaton
        count[100], limit[100], active[100] = L, 99, True              # beyond the history: the same
    else:
        active[0], limit[0] = True, 12
    # the global mask: every symbol but the last (so the intersection matters), plus bystanders no automaton permits
    allow_bool = torch.zeros(512, dtype=torch.bool)
    allow_bool[ids[:-1] if n_sym > 1 else ids] = True
    allow_bool[[3, 100, 509]] = True
    rows_cpu = torch.randn(L, S, 512, generator=g) * 3.0
    rows_cpu = rows_cpu if f32 else rows_cpu.bfloat16()
    stop_bool = H.allowed_mask(None, [ids[0]]) if n_sym > 1 else None
    case = Case(S, ids, table, base, state, limit, active, count, rows_cpu, allow_bool, stop_bool, [[ids[1], ids[1]]] if n_sym > 1 else [], 1)
    final, seen = case.run()
    print(f"[dfa kernel S={S} {alphabet}] finishes seen: {sorted({f for f, _ in seen})}")
    if S == 257:
        reasons = {f for f, _ in seen}
        assert H.FINISH_DEAD_END in reasons and H.FINISH_LENGTH in reasons and (H.FINISH_LENGTH, "no draw") in seen
        if n_sym > 1:
            assert H.FINISH_CONSTRAINT in reasons and H.FINISH_STOP_TOKEN in reasons
        for r in (10, 14, 18):                                        # dead ends: nothing drawn, the state stays
            assert int(base[r]) == 27 and final[r][:2] == (0, H.FINISH_DEAD_END) and int(case.final["ids"][r]) == -7
        assert final[10][2] == 13 and final[14][2] == -1 and final[18][2] == 2 ** 30
        assert bool((case.final["state"].cpu()[base < 0] == STATE_CANARY).all())
        assert final[100][:2] == (L, H.FINISH_LENGTH)


def test_kernel_scripted_rows():
    """Every row puts +60 on the token of its script; what each one shows stands beside it."""
    chain12, chain8, chain1 = "ACACACACACAC", "CAACAACA", "G"
    only_a = "AAAAAAAAAAAA"
    parts = [K.iupac_template(chain12).table, K.iupac_template(chain8).table, K.iupac_template(chain1).table, K.iupac_template(only_a).table,
             np.full((1, 8), -1, dtype=np.int32),                    # a state that permits nothing
             K.iupac_template("AT").table, K.iupac_template("CAC").table, K.iupac_template("GG").table,
             np.array([[-2, 0, -1, -1, -1, -1, -1, -1]], dtype=np.int32)]          # the LAST row of the table: A accepts, C stays
    offs = np.cumsum([0] + [len(p) for p in parts]).tolist()
    table = torch.from_numpy(np.concatenate(parts))
    n_states = table.shape[0]
    assert offs[-1] == n_states and offs[8] == n_states - 1
    #        script          base      state  limit  active   expected (length, finish)
    rows = [(chain12,        offs[0],  0,     12,    True,    (12, 4)),       # accepts at n = 12 = its limit: reason 4 outranks 3
            (chain8 + "AAAA", offs[1], 0,     12,    True,    (8, 4)),        # accepts at n = 8
            (chain1 + "A" * 11, offs[2], 0,   12,    True,    (1, 4)),        # accepts on its first token
            ("T" * 12,       offs[3],  0,     12,    True,    (12, 4)),       # +60 on the forbidden T every time: only A is ever drawn
            ("CCCA" + "A" * 8, offs[8], 0,    12,    True,    (4, 4)),        # its state is the last row of the table
            ("C" * 12,       -1,       0,     12,    True,    (12, 3)),       # base < 0: free, ends by length; dfa_state untouched
            ("A" * 12,       offs[4],  0,     12,    True,    (0, 5)),        # dead end: no draw
            ("A" * 12,       offs[2],  n_states, 12, True,    (0, 5)),        # dfa_state points past n_states
            ("A" * 12,       offs[0],  0,     12,    False,   (-5, 9)),       # inactive: nothing of it may change
            ("AT" + "A" * 10, offs[5], 0,     12,    True,    (2, 1)),        # accepts on the stop token T: reason 1 wins
            ("CAC" + "A" * 9, offs[6], 0,     3,     True,    (3, 4)),        # accepts at its limit 3: reason 4 wins
            ("GG" + "A" * 10, offs[7], 0,     12,    True,    (2, 2)),        # accepts on the token that completes the pattern GG: reason 2 wins
            ("AAC" + "A" * 9, offs[0], 0,     12,    True,    None)]          # chain12 wants C second: +60 on a forbidden A there, C is drawn
    S = len(rows)
    for f32 in (False, True):
        g = torch.Generator().manual_seed(5 + f32)
        x = (torch.randn(L, S, 512, generator=g) * 3.0).bfloat16()
        for s, r in enumerate(rows):
            for t in range(L):
                x[t, s, ord(r[0][t])] = 60.0
        state = torch.tensor([r[2] for r in rows], dtype=torch.int32)
        state[5] = STATE_CANARY
        case = Case(S, [A, C, G, T], table, torch.tensor([r[1] for r in rows], dtype=torch.int64), state,
                    torch.tensor([r[3] for r in rows], dtype=torch.int64), torch.tensor([r[4] for r in rows]), torch.zeros(S, dtype=torch.int64),
                    x.float() if f32 else x, acgt_mask(), H.allowed_mask(None, [T]), [[G, G]], 1)
        final, _ = case.run()
        for s, r in enumerate(rows):
            if r[5] is not None:
                assert final[s][:2] == r[5], (s, final[s], r)
        hid = case.final["hid"].cpu()
        assert "".join(chr(t) for t in hid[0].tolist()) == chain12 and "".join(chr(t) for t in hid[3].tolist()) == only_a
        assert "".join(chr(t) for t in hid[4, :4].tolist()) == "CCCA" and T not in hid[3].tolist()
        assert final[5][2] == STATE_CANARY and final[7][2] == n_states and final[6][2] == 0
        assert hid[12, :3].tolist() == [A, C, A] and final[12][:2] == (12, 4)       # the forbidden A was never drawn second
        assert bool((hid[[6, 7, 8]] == -9).all()) and case.final["ids"].cpu()[[6, 7, 8]].tolist() == [-7] * 3


def test_one_element_slices_at_an_odd_slot():
    """The pool's fill(): ONE slot sampled through one-element slices of the per-slot vectors (element alignment only)."""
    S, slot = 6, 3
    g = torch.Generator().manual_seed(9)
    c = K.encode_protein("MLS*")
    rows_cpu = (torch.randn(L, S, 512, generator=g) * 3.0).bfloat16()
    mk = lambda: Case(S, c.alphabet, torch.from_numpy(c.table), torch.zeros(S, dtype=torch.int64), torch.zeros(S, dtype=torch.int32),
                      torch.full((S,), 12, dtype=torch.int64), torch.ones(S, dtype=torch.bool), torch.zeros(S, dtype=torch.int64), rows_cpu,
                      acgt_mask(), None, [], 1)
    whole = mk()
    whole.run()
    one = mk()
    one.limit_dev, one.base_dev = one.limit.to(DEV), one.base.to(DEV)
    st = one.device_state()
    for t in range(L):
        one.launch(st, t, slice(slot, slot + 1))
    torch.cuda.synchronize()
    fresh = one.device_state()
    for k, v in st.items():
        assert torch.equal(v[slot], whole.final[k][slot]), k          # the slot: what the whole launch gave it
        keep = [s for s in range(S) if s != slot]
        assert torch.equal(v[keep], fresh[k][keep]), k                # every other slot: untouched
    assert int(st["finish"][slot]) == H.FINISH_CONSTRAINT and int(st["length"][slot]) == 12


# ------------------------------------------------------------------------------------------------ arena
@covers("evo_sample_rows_dfa_f32")
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("hist", ["all", "ids", "none"])
def test_sample_rows_dfa_in_the_arena(hist, f32):
    """S = 6: a row at cnt = 0, a row in mid-history, an inactive row, a row with nothing left to draw, a row at the last cell whose state
    is the LAST row of the table (the table is carved last: behind it lie only its guard band and the arena's end), a free row.  Per-row
    vectors at their element's alignment, the table at 16 bytes."""
    o, g = ops(), gen(6)
    S, Lh = 6, 9
    c = K.open_reading_frame(2)
    table = torch.from_numpy(np.concatenate([c.table, np.array([[0, 0, 0, -2, 7, 7, 7, 7]], dtype=np.int32)]))
    last = table.shape[0] - 1
    alpha = torch.tensor(c.alphabet, dtype=torch.int32)
    stop_seq = o.pack_stop_sequences([[A, C, G, T, A, C, G, A], [C] * 8, [G]]) if hist != "none" else None
    inp = {"lg": rnd((S, 520), g, 3.0, torch.float32 if f32 else torch.bfloat16), "top_k": torch.full((S,), 4, dtype=torch.int32, device=DEV),
           "top_p": torch.full((S,), 0.9, dtype=torch.float32, device=DEV), "temp": torch.full((S,), 0.7, dtype=torch.float32, device=DEV),
           "stream": torch.arange(S, dtype=torch.int64, device=DEV) * 3 + 1,
           "count": torch.tensor([0, 2, 1, 4, Lh - 1, 3], dtype=torch.int64, device=DEV),
           "active": torch.tensor([True, True, False, True, True, True], device=DEV),
           "limit": torch.tensor([9, 3, 9, 4, 9, 9], dtype=torch.int64, device=DEV),
           "allow": o.pack_allow_mask(acgt_mask(), DEV), "stop_mask": o.pack_allow_mask(H.allowed_mask(None, [T]), DEV),
           "ids": poisoned((S,), torch.int64), "lp": poisoned((S,), torch.float32), "length": poisoned((S,), torch.int64),
           "finish": poisoned((S,), torch.uint8),
           "base": torch.tensor([0, 0, 0, 0, last, -1], dtype=torch.int64, device=DEV),
           "state": torch.tensor([0, 2, 0, 1, 0, STATE_CANARY], dtype=torch.int32, device=DEV)}
    if hist != "none":
        inp["hist_ids"] = poisoned((S, Lh), torch.int64)
    if hist == "all":
        inp["hist_logits"] = poisoned((S, Lh, 512), torch.float32)
        inp["hist_logprob"] = poisoned((S, Lh), torch.float32)
    inp["dfa_next"] = table.to(DEV)                                   # carved last

    def fn(lg, top_k, top_p, temp, stream, count, active, limit, allow, stop_mask, ids, lp, length, finish, base, state, dfa_next, hist_ids=None,
           hist_logits=None, hist_logprob=None):
        o.sample_rows_dfa(lg[:, :512], top_k, top_p, temp, 1234, count=count, active=active, limit=limit, length=length, finish=finish,
                          dfa_alphabet=alpha, dfa_next=dfa_next, dfa_base=base, dfa_state=state, stream=stream, allow=allow, ids_out=ids,
                          logprob_out=lp, hist_ids=hist_ids, hist_logits=hist_logits, hist_logprob=hist_logprob, stop_mask=stop_mask,
                          stop_seq=stop_seq, stop_frame=1)
    run = _run(fn, inp, inout=["count", "active", "ids", "lp", "length", "finish", "state"] + [k for k in inp if k.startswith("hist_")],
               expect=["evo_sample_rows_dfa_f32"],
               align={"top_k": 4, "top_p": 4, "temp": 4, "stream": 8, "count": 8, "active": 1, "limit": 8, "ids": 8, "lp": 4, "length": 8,
                      "finish": 1, "hist_ids": 8, "hist_logprob": 4, "base": 8, "state": 4})
    got = run.inputs
    assert got["count"].tolist() == [1, 3, 1, 4, Lh, 4] and is_poison(got["ids"][2]) and is_poison(got["ids"][3]) and is_poison(got["lp"][3])
    assert int(got["ids"][0]) == A and int(got["state"][0]) == 1      # the ORF's first state permits A alone
    assert int(got["state"][2]) == 0 and int(got["state"][3]) == 1 and int(got["state"][5]) == STATE_CANARY
    assert got["active"].tolist()[1:5] == [False] * 4                 # limit 3 reached, inactive, exhausted, last cell = limit 9
    assert int(got["length"][1]) == 3 and int(got["length"][3]) == 4 and int(got["length"][4]) == Lh and is_poison(got["length"][2])
    assert int(got["finish"][3]) == 3 and int(got["finish"][1]) in (2, 3) and int(got["finish"][4]) in (1, 2, 3, 4)
    assert (int(got["finish"][4]) in (1, 4)) == (int(got["ids"][4]) == T)           # T accepts in the last table row (and is the stop token)
    assert bool(got["active"][0]) and is_poison(got["length"][0]) and is_poison(got["finish"][0])
    if hist != "none":
        hid = got["hist_ids"]
        assert int(hid[0, 0]) == int(got["ids"][0]) and int(hid[1, 2]) == int(got["ids"][1]) and int(hid[4, Lh - 1]) == int(got["ids"][4])
        assert is_poison(hid[2]) and is_poison(hid[3]) and is_poison(hid[0, 1:]) and is_poison(hid[4, : Lh - 1])
    if hist == "all":
        assert is_poison(got["hist_logits"][3]) and is_poison(got["hist_logits"][0, 1:]) and not is_poison(got["hist_logits"][0, 0])
        assert torch.equal(got["hist_logprob"][[0, 1, 4], [0, 2, Lh - 1]], got["lp"][[0, 1, 4]])


# ------------------------------------------------------------------------------------------------ pool
N_JOBS = len(PROMPTS) * N_SPP
_RUNS = {}


def toy():
    """The toy model of tests/test_gpu_stop.py (its weights' seed leaves the samples some variety) and its tokenizer."""
    if "model" not in _RUNS:
        from evo_amd.tokenizer import CharLevelTokenizer
        cfgd = dict(SMALL4, use_interpolated_rotary_pos_emb=True, rotary_emb_scaling_factor=16)
        _RUNS["model"] = (build(cfgd, seed=WEIGHTS_SEED)[2], CharLevelTokenizer(512))
    return _RUNS["model"]


def make_pool(use_graph=True, **kw):
    from evo_amd.pool import DecodePool
    m, tok = toy()
    return DecodePool(m, tok, n_slots=4, device=DEV, use_graph=use_graph, seed=POOL_SEED, allowed_tokens="ACGT", **SET, **kw)


def result(pool, out):
    """What a finished run leaves, detached from the pool."""
    return SimpleNamespace(seqs=out[0], scores=out[1], owner=out[2], last_ids=pool.last_ids, last_logits=pool.last_logits,
                           last_logprobs=getattr(pool, "last_logprobs", None), last_lengths=getattr(pool, "last_lengths", None),
                           last_finish=getattr(pool, "last_finish", None), stats=dict(pool.stats), captured=pool._graph is not None,
                           kept_logits=pool.hist_logits is not None, idle=not bool(pool.s_active.any()),
                           table_shape=tuple(pool.s_dfa_next.shape) if pool.s_dfa_next is not None else None,
                           store=(list(pool.store_refs), pool.store.row.tolist()) if pool.store is not None else None)


def run(name, constraints, n_tokens, use_graph=True, return_logits=True, sampling=None, **kw):
    """One pool run: 4 slots, PROMPTS x 3, ACGT only, seeded.  Its results are cached by name; the pool and its graph are dropped."""
    if name not in _RUNS:
        pool = make_pool(use_graph, **kw)
        gen_kw = {} if constraints is None else {"constraints": constraints}
        if sampling is not None:
            gen_kw["sampling"] = [sampling] * len(PROMPTS)
        if not return_logits:
            gen_kw["return_logits"] = False
        _RUNS[name] = result(pool, pool.generate(PROMPTS, n_tokens=n_tokens, n_sample_per_prompt=N_SPP, **gen_kw))
        del pool
        gc.collect()
    return _RUNS[name]


def same(p, q):
    return (torch.equal(p.last_ids, q.last_ids) and torch.equal(p.last_logprobs, q.last_logprobs) and p.last_lengths == q.last_lengths
            and p.last_finish == q.last_finish and p.seqs == q.seqs and p.scores == q.scores)


def translate(dna):
    return "".join(CODE[dna[i:i + 3]] for i in range(0, len(dna) - len(dna) % 3, 3))


def test_pool_under_an_all_n_template_is_the_unconstrained_run_bit_for_bit():
    F = run("fixed length", None, 12)                                 # the fixed-length path: evo_sample_rows_f32
    U = run("free", None, [12] * len(PROMPTS))                        # the job-control path without constraints: log-probabilities
    P = run("N12", K.iupac_template("N" * 12), 12)
    assert F.last_lengths is None and U.table_shape is None
    assert torch.equal(P.last_ids, F.last_ids) and torch.equal(P.last_logits, F.last_logits) and P.seqs == F.seqs
    assert torch.equal(P.last_ids, U.last_ids) and torch.equal(P.last_logprobs, U.last_logprobs) and torch.equal(P.last_logits, U.last_logits)
    assert P.seqs == U.seqs and P.scores == U.scores and P.owner == [pi for pi in range(len(PROMPTS)) for _ in range(N_SPP)]
    assert P.last_finish == ["constraint"] * N_JOBS and P.last_lengths == [12] * N_JOBS and U.last_finish == ["length"] * N_JOBS
    assert P.stats["constraint_ends"] == N_JOBS and P.stats["length_ends"] == 0 and P.stats["stop_ends"] == 0
    assert P.stats["steps"] == U.stats["steps"] and P.stats["polls"] > 0 and P.idle and P.captured


def test_pool_templates_proteins_and_reading_frames():
    fixed = "ATGCGTACGTAA"
    P = run("fixed", K.iupac_template(fixed), 20)
    assert P.seqs == [fixed] * N_JOBS and P.last_finish == ["constraint"] * N_JOBS
    for j in range(N_JOBS):                                           # the scores are those of the forced tokens under the model
        assert P.scores[j] == float(np.mean(P.last_logprobs[j, :12].numpy().astype(np.float64))) and bool((P.last_ids[j, 12:] == -1).all())
    c = K.encode_protein("MKLS*")
    P = run("protein", c, 20)
    assert all(len(s) == 15 and translate(s) == "MKLS*" and c.accepts(s) for s in P.seqs), P.seqs
    assert P.last_finish == ["constraint"] * N_JOBS and P.stats["constraint_ends"] == N_JOBS
    print(f"[constraints protein] {sorted(set(P.seqs))}")
    orf = K.open_reading_frame(3)
    # at the pool's own temperature, and at T = 8 through per-prompt `sampling` (the toy model's samples at T = 1 are close to
    # homopolymer runs, tests/test_gpu_stop.py: few stop codons; a high temperature spreads the draws)
    for name, sampling in (("orf", None), ("orf hot", {"temperature": 8.0})):
        P = run(name, orf, 60, sampling=sampling)
        ended = 0
        for j, s in enumerate(P.seqs):
            codons = [s[i:i + 3] for i in range(0, len(s) - 2, 3)]
            assert s.startswith("ATG") and orf.walk(s) != K.FORBIDDEN, s
            if P.last_finish[j] == "constraint":
                assert orf.accepts(s) and len(s) % 3 == 0 and len(codons) >= 3 and codons[-1] in STOPS and not any(k in STOPS for k in codons[:-1]), s
                ended += 1
            else:
                assert P.last_finish[j] == "length" and len(s) == 60 and not any(k in STOPS for k in codons), s
        print(f"[constraints {name}] {ended} of {N_JOBS} reading frames closed, lengths {P.last_lengths}")
        assert P.stats["constraint_ends"] == ended and P.stats["length_ends"] == N_JOBS - ended


def test_pool_graph_equals_eager_and_the_run_without_logits():
    c = K.encode_protein("MKLS*")
    P = run("protein", c, 20)
    E = run("protein eager", c, 20, use_graph=False)
    assert P.captured and not E.captured
    assert same(P, E) and torch.equal(P.last_logits, E.last_logits)
    Q = run("protein scores only", c, 20, return_logits=False)
    assert Q.last_logits is None and not Q.kept_logits and same(P, Q)
    # one pool called again with another constraint of the same size replays its captured step on the new table
    pool = make_pool()
    first = pool.generate(PROMPTS, n_tokens=20, n_sample_per_prompt=N_SPP, constraints=c)
    graph, table = pool._graph, pool.s_dfa_next
    seqs, _, _ = pool.generate(PROMPTS, n_tokens=20, n_sample_per_prompt=N_SPP, constraints=K.encode_protein("MNLS*"))
    assert pool._graph is graph and graph is not None and pool.s_dfa_next is table and all(translate(s) == "MNLS*" for s in seqs), seqs
    again = pool.generate(PROMPTS, n_tokens=20, n_sample_per_prompt=N_SPP, constraints=c)
    assert again == first and first[0] == P.seqs and first[1] == P.scores
    # the pool's graph lives: a capture OUTSIDE inference mode still works (the pool begins its own captures outside it, so the capture
    # state torch's generator keeps while any graph lives is no inference tensor)
    x = torch.zeros(4, device=DEV)
    other = torch.cuda.CUDAGraph()
    with torch.cuda.graph(other):
        x.add_(1.0)
    other.replay()
    torch.cuda.synchronize()
    assert x.tolist() == [1.0] * 4 and pool._graph is graph
    del other
    del pool, graph
    gc.collect()


def test_pool_mixes_constrained_and_free_prompts():
    """A free job beside constrained ones is the job of the unconstrained run (a row's logits do not depend on its neighbours at a fixed
    slot count: tests/test_gpu_pool_seeded.py), a constrained one obeys its own automaton."""
    U = run("free", None, [12] * len(PROMPTS))
    tpl, prot = K.iupac_template("ATGNNNRRYTAA"), K.encode_protein("MW*")
    cons = [tpl, None, prot, None, tpl, None]
    P = run("mixed", cons, 12)
    assert P.table_shape == (tpl.n_states + prot.n_states, 8)        # the distinct automata, once each
    for j, s in enumerate(P.seqs):
        c = cons[P.owner[j]]
        if c is None:
            assert P.last_finish[j] == "length" and torch.equal(P.last_ids[j], U.last_ids[j]) and torch.equal(P.last_logprobs[j], U.last_logprobs[j])
        else:
            assert P.last_finish[j] == "constraint" and c.accepts(s), (j, s)
    assert [translate(P.seqs[j]) for j in range(6, 9)] == ["MW*"] * 3 and P.stats["constraint_ends"] == 9 and P.stats["length_ends"] == 9


@pytest.mark.parametrize("option", ["share_prompt_kv", "prefill_batch"])
def test_pool_combinations(option):
    """share_prompt_kv / prefill_batch change the attention and prefill kernels: nothing is compared across paths; every output obeys its
    constraint, and two runs are identical."""
    kw = {"share_prompt_kv": True} if option == "share_prompt_kv" else {"prefill_batch": 2}
    c = K.concat(K.iupac_template("ATGNNN"), K.encode_protein("LS*"))
    P = run(option, c, 20, **kw)
    assert all(len(s) == 15 and c.accepts(s) and translate(s[6:]) == "LS*" for s in P.seqs), P.seqs
    assert P.last_finish == ["constraint"] * N_JOBS and P.idle
    if option == "share_prompt_kv":
        assert P.store == ([0] * len(P.store[0]), [-1] * 4)
    else:
        assert P.stats["prefills"] < len(PROMPTS)
    assert same(P, run(option + " again", c, 20, **kw))
