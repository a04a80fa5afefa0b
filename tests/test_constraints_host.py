"""CPU: constrained generation by per-job token automata -- the layers that need no GPU.

  * the builders (evo_amd/constraints.py) against enumeration: the language each automaton accepts is computed here by brute force over
    every ACGT string, with an independent 64-entry genetic code written below;
  * `validate` / `min_length`;
  * the written rule (evo_amd/sh/sample.py: dfa_allowed, sample_dfa) against `sample_ctl` with the state's set as its allow mask, the
    priority of the finish reasons 1 > 2 > 4 > 3, a dead end, an unconstrained row;
  * the C entry evo_sample_rows_dfa_f32: exported, declared, bound, ABI >= 18, every contract violation refused with -1 before any launch;
  * the scheduler of DecodePool on the fp64 oracle backend with `sample_rows_dfa` written from the specification: constrained and free
    prompts of unequal limits mixed at 3 slots, every job equal to a one-job-at-a-time loop written here;
  * resources: the automaton kernel without scratch or spills, in the LDS of the plain sampler."""
import ctypes
import os
import re
from itertools import product
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import evo_amd
from evo_amd import _build
from evo_amd import constraints as K
from evo_amd import ops as evo_ops
from evo_amd.pool import DecodePool, sample_many
from evo_amd.sh import sample as H
from test_kernel_resources import HIPCC, _metadata
from test_stop_host import PROMPTS, SMALL, TOK, CtlOracleOps, _bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, C, G, T = (ord(c) for c in "ACGT")
ACGT = (A, C, G, T)

# the standard genetic code, codon by codon (independent of the 64-letter string of evo_amd/constraints.py)
CODE = {"TTT": "F", "TTC": "F", "TTA": "L", "TTG": "L", "CTT": "L", "CTC": "L", "CTA": "L", "CTG": "L", "ATT": "I", "ATC": "I", "ATA": "I",
        "ATG": "M", "GTT": "V", "GTC": "V", "GTA": "V", "GTG": "V", "TCT": "S", "TCC": "S", "TCA": "S", "TCG": "S", "CCT": "P", "CCC": "P",
        "CCA": "P", "CCG": "P", "ACT": "T", "ACC": "T", "ACA": "T", "ACG": "T", "GCT": "A", "GCC": "A", "GCA": "A", "GCG": "A", "TAT": "Y",
        "TAC": "Y", "TAA": "*", "TAG": "*", "CAT": "H", "CAC": "H", "CAA": "Q", "CAG": "Q", "AAT": "N", "AAC": "N", "AAA": "K", "AAG": "K",
        "GAT": "D", "GAC": "D", "GAA": "E", "GAG": "E", "TGT": "C", "TGC": "C", "TGA": "*", "TGG": "W", "CGT": "R", "CGC": "R", "CGA": "R",
        "CGG": "R", "AGT": "S", "AGC": "S", "AGA": "R", "AGG": "R", "GGT": "G", "GGC": "G", "GGA": "G", "GGG": "G"}
STOPS = ("TAA", "TAG", "TGA")


def strings(max_len, min_len=1):
    for n in range(min_len, max_len + 1):
        for s in product("ACGT", repeat=n):
            yield "".join(s)


def translate(dna):
    return "".join(CODE[dna[i:i + 3]] for i in range(0, len(dna), 3))


def accepted(c, max_len):
    return {s for s in strings(max_len) if c.accepts(s)}


def language(c, max_len):
    """Every string of at most max_len tokens that ends on an ACCEPT edge, by a depth-first walk of the table itself."""
    out, todo = set(), [(0, "")]
    while todo:
        q, s = todo.pop()
        for a, t in enumerate(c.alphabet):
            nxt = int(c.table[q, a])
            if nxt == K.ACCEPT:
                out.add(s + chr(t))
            elif nxt >= 0 and len(s) + 1 < max_len:
                todo.append((nxt, s + chr(t)))
    return out


# ------------------------------------------------------------------------------------------------ builders against enumeration
def test_iupac_template_accepts_the_product_of_its_sets():
    c = K.iupac_template("RYN").validate()
    assert accepted(c, 4) == {r + y + n for r in "AG" for y in "CT" for n in "ACGT"}
    assert c.alphabet == ACGT and c.table.dtype == np.int32 and c.table.shape == (3, 8) and c.min_length() == 3
    assert bool((c.table[:, 4:] == K.FORBIDDEN).all())
    every = K.iupac_template("ACGTRYSWKMBDHVN")
    assert every.min_length() == 15 and every.accepts("ACGTACCAGACAAAA") and not every.accepts("ACGTACCAGACAAA")
    for code, letters in K.IUPAC.items():
        assert accepted(K.iupac_template(code), 2) == set(letters), code
    for bad in ("ACGU", "acgt", "AC-T", ""):
        with pytest.raises(ValueError):
            K.iupac_template(bad)
    with pytest.raises(ValueError):
        K.iupac_template("ACGT", then="stop")


def test_encode_protein_accepts_exactly_the_dna_that_translates_to_it():
    c = K.encode_protein("MLS*").validate()
    codons = {aa: [k for k, v in CODE.items() if v == aa] for aa in "MLS*"}
    want = {"".join(w) for w in product(*(codons[aa] for aa in "MLS*"))}
    assert len(want) == 1 * 6 * 6 * 3 == 108 and all(translate(s) == "MLS*" for s in want)
    assert language(c, 16) == want and all(c.accepts(s) for s in want)
    # every string of a shorter protein, by brute force: accepted <=> it translates to the protein
    short = K.encode_protein("S*")
    assert accepted(short, 7) == {s for s in strings(6, 6) if translate(s) == "S*"} == language(short, 7)
    assert not any(c.accepts(s) for s in strings(6)) and c.min_length() == 12
    assert c.n_states <= 21 * 4                                       # a root, first letters, two-letter prefixes per residue
    assert K.encode_protein("L").n_states == 1 + 2 + 2 and K.encode_protein("M").n_states == 3
    assert accepted(K.encode_protein("*"), 3) == set(STOPS)
    for bad in ("MXL", "mk", "M L", "", "B"):
        with pytest.raises(ValueError):
            K.encode_protein(bad)


def test_genetic_code_is_the_standard_one():
    assert K.GENETIC_CODE == CODE and len(K.GENETIC_CODE) == 64
    count = {aa: len(K.codons_of(aa)) for aa in set(CODE.values())}
    assert (count["L"], count["S"], count["R"], count["*"], count["M"], count["W"]) == (6, 6, 6, 3, 1, 1)
    assert sum(count.values()) == 64 and len(count) == 21
    assert sorted(K.codons_of("*")) == sorted(STOPS) and K.codons_of("M") == ["ATG"]


def orf_rule(s, start, min_codons):
    codons = [s[i:i + 3] for i in range(0, len(s), 3)]
    return (len(s) % 3 == 0 and len(s) >= 3 and (start is None or s.startswith(start)) and codons[-1] in STOPS
            and not any(c in STOPS for c in codons[:-1]) and len(codons) >= min_codons)


def test_open_reading_frame_against_the_rule_on_every_string():
    c = K.open_reading_frame(2, "ATG").validate()
    for s in strings(9):
        # the issue's rule: starts with ATG, whole codons, the last codon is a stop, no earlier in-frame codon is one
        want = s.startswith("ATG") and len(s) % 3 == 0 and s[-3:] in STOPS and not any(s[i:i + 3] in STOPS for i in range(0, len(s) - 3, 3))
        assert c.accepts(s) == want == orf_rule(s, "ATG", 2), s
    assert c.min_length() == 6
    # before codon `min_codons` the edge that would complete a stop codon is forbidden; from there on it accepts
    c3 = K.open_reading_frame(3, None).validate()
    for s in strings(9):
        assert c3.accepts(s) == orf_rule(s, None, 3), s
    assert c3.walk("TA") >= 0 and c3.walk("TAA") == K.FORBIDDEN and c3.walk("TAC") >= 0 and c3.walk("CCCTGA") == K.FORBIDDEN
    assert c3.walk("CCCCCCTGA") == K.ACCEPT and c3.min_length() == 9
    # the states come from the prefixes of the stop codons given, not from T / TA / TG
    amber = K.open_reading_frame(1, None, stops=("CAG",)).validate()
    assert accepted(amber, 6) == {"CAG"} | {a + "CAG" for a in strings(3, 3) if a != "CAG"}
    assert K.open_reading_frame(50).min_length() == 150
    for bad in (dict(min_codons=0), dict(min_codons=2, start="AT"), dict(min_codons=2, stops=("TA",)), dict(min_codons=2, stops=()),
                dict(min_codons=2, start="TAA")):
        with pytest.raises(ValueError):
            K.open_reading_frame(**bad)


def test_concat_and_free_continuations():
    c = K.concat(K.iupac_template("AC"), K.open_reading_frame(1, None)).validate()
    assert accepted(c, 8) == {"AC" + s for s in strings(6) if orf_rule(s, None, 1)}
    assert c.min_length() == 5 and c.n_states == 2 + K.open_reading_frame(1, None).n_states
    two = K.concat(K.encode_protein("M"), K.iupac_template("RY"))
    assert accepted(two, 6) == {"ATG" + r + y for r in "AG" for y in "CT"}
    with pytest.raises(ValueError):
        K.concat(K.iupac_template("A"), K.TokenConstraint([A, C, G], [[-2, -2, -2]]))
    # then="free": never accepts, every continuation is permitted behind the constraint
    for free in (K.iupac_template("RY", then="free"), K.encode_protein("M*", then="free")):
        free.validate()
        assert free.min_length() is None and not any(free.accepts(s) for s in strings(8))
    f = K.iupac_template("RY", then="free")
    assert f.walk("AC") == f.walk("ACGGTTAACC") >= 0 and f.walk("CC") == K.FORBIDDEN
    # a free constraint followed by another: the second is never reached, and that is not an error
    assert K.concat(f, K.iupac_template("A")).validate().min_length() is None
    assert evo_amd.iupac_template is K.iupac_template and evo_amd.TokenConstraint is K.TokenConstraint
    assert evo_amd.encode_protein is K.encode_protein and evo_amd.open_reading_frame is K.open_reading_frame and evo_amd.concat is K.concat


# ------------------------------------------------------------------------------------------------ validate
def test_validate():
    ok = K.TokenConstraint(ACGT, [[1, -1, -1, -1], [-2, -2, -1, -1]]).validate()
    assert ok.min_length() == 2 and ok.accepts([A, C]) and not ok.accepts([C, A]) and ok.walk([A]) == 1
    for bad in (2, 7, -3, -100):                                      # a transition outside [0, n) that is neither ACCEPT nor FORBIDDEN
        with pytest.raises(ValueError, match="outside"):
            K.TokenConstraint(ACGT, [[1, -1, -1, -1], [bad, -2, -1, -1]]).validate()
    with pytest.raises(ValueError, match="permits no token"):         # a reachable dead end
        K.TokenConstraint(ACGT, [[1, -1, -1, -1], [-1, -1, -1, -1]]).validate()
    for bad in (2, -3):                                               # the constructor refuses it too; a table written to later: validate
        with pytest.raises(ValueError, match="outside"):
            K.TokenConstraint(ACGT, [[1, -1, -1, -1], [bad, -2, -1, -1]])
        late = K.TokenConstraint(ACGT, [[1, -1, -1, -1], [-2, -2, -1, -1]])
        late.table[1, 0] = bad
        with pytest.raises(ValueError, match="outside"):
            late.validate()
    unreachable = K.TokenConstraint(ACGT, [[-2, 0, -1, -1], [-1, -1, -1, -1]])
    assert unreachable.validate() is unreachable                      # state 1 permits nothing, and nothing leads to it
    # a dead end that exists only once T may not be drawn: position 0 of TAA, and the T-only state behind "AC"
    for c in (K.iupac_template("TAA"), K.iupac_template("ACT")):
        c.validate()
        c.validate("ACGT")
        with pytest.raises(ValueError, match="among the allowed"):
            c.validate("ACG")
        with pytest.raises(ValueError, match="among the allowed"):
            c.validate(H.allowed_mask(TOK, "ACG"))
    K.iupac_template("ACN").validate("ACG")                           # N without T still has three letters
    # ... and one that the allowed set makes unreachable
    K.TokenConstraint(ACGT, [[-2, -1, -1, 1], [-1, -1, -1, -1]]).validate("ACG")
    for bad in ((), (A, A), (512,), (-1,), tuple(range(9))):
        with pytest.raises(ValueError):
            K.TokenConstraint(bad, np.zeros((1, 8), dtype=np.int32))
    with pytest.raises(ValueError):
        K.TokenConstraint(ACGT, np.zeros((0, 8), dtype=np.int32))
    assert K.TokenConstraint(ACGT, [[0, 0, 0, 0]]).min_length() is None


# ------------------------------------------------------------------------------------------------ the rule
def _row(seed=0):
    return torch.randn(512, generator=torch.Generator().manual_seed(seed)) * 3


def test_sample_dfa_is_sample_ctl_on_the_states_set():
    assert (H.FINISH_CONSTRAINT, H.FINISH_DEAD_END, H.DFA_ACCEPT) == (4, 5, -2) == (4, 5, K.ACCEPT)
    assert H.FINISH_NAMES_ALL == {1: "stop_token", 2: "stop_sequence", 3: "length", 4: "constraint", 5: "dead_end"}
    c = K.encode_protein("LS*")
    allowed = H.allowed_mask(TOK, "ACGT")
    for q in range(c.n_states):
        mask = H.dfa_allowed(c.table, q, c.alphabet)
        assert set(torch.nonzero(mask).flatten().tolist()) == {t for a, t in enumerate(ACGT) if c.table[q, a] >= 0 or c.table[q, a] == -2}
        for seed in range(3):
            row, hist = _row(seed + 10 * q), [A] * seed
            tok, n, fin, new = H.sample_dfa(row, 0, 1.0, 2.0, 5, 7, hist, 99, c.table, q, c.alphabet, allowed)
            assert (tok, n) == H.sample_ctl(row, 0, 1.0, 2.0, 5, 7, hist, 99, mask)[:2] and bool(mask[tok])
            nxt = int(c.table[q, ACGT.index(tok)])
            assert (fin, new) == ((H.FINISH_CONSTRAINT, q) if nxt == -2 else (0, nxt))
    assert not bool(H.dfa_allowed(c.table, c.n_states, c.alphabet).any()) and not bool(H.dfa_allowed(c.table, -1, c.alphabet).any())
    # the global mask intersects: L's root permits C and T; without T only C is left
    assert torch.nonzero(H.dfa_allowed(c.table, 0, c.alphabet, H.allowed_mask(TOK, "ACG"))).flatten().tolist() == [C]
    # a base: the same automaton behind 5 other rows of the table
    table = np.concatenate([np.full((5, 8), -1, dtype=np.int32), c.table])
    row = _row(3)
    assert H.sample_dfa(row, 0, 1.0, 2.0, 5, 7, [], 99, table, 2, c.alphabet, base=5) == H.sample_dfa(row, 0, 1.0, 2.0, 5, 7, [], 99, c.table, 2, c.alphabet)


def test_finish_priority_dead_ends_and_free_rows():
    one = K.iupac_template("A")                                       # state 0: A accepts
    row = _row(1)
    assert H.sample_dfa(row, 4, 1.0, 1.0, 5, 7, [], 9, one.table, 0, one.alphabet) == (A, 1, H.FINISH_CONSTRAINT, 0)
    # 1 > 4: the accepting token is a stop token;  2 > 4: it completes an in-frame pattern;  4 > 3: acceptance at the limit
    assert H.sample_dfa(row, 4, 1.0, 1.0, 5, 7, [], 9, one.table, 0, one.alphabet, stop_tokens={A})[2] == H.FINISH_STOP_TOKEN
    assert H.sample_dfa(row, 4, 1.0, 1.0, 5, 7, [C], 9, one.table, 0, one.alphabet, stop_sequences=[[C, A]], stop_frame=2)[2] == H.FINISH_STOP_SEQUENCE
    assert H.sample_dfa(row, 4, 1.0, 1.0, 5, 7, [C], 9, one.table, 0, one.alphabet, stop_sequences=[[C, A]], stop_frame=3)[2] == H.FINISH_CONSTRAINT
    assert H.sample_dfa(row, 4, 1.0, 1.0, 5, 7, [], 1, one.table, 0, one.alphabet)[2] == H.FINISH_CONSTRAINT
    two = K.iupac_template("AA")
    assert H.sample_dfa(row, 4, 1.0, 1.0, 5, 7, [], 1, two.table, 0, two.alphabet) == (A, 1, H.FINISH_LENGTH, 1)
    assert H.sample_dfa(row, 4, 1.0, 1.0, 5, 7, [], 9, two.table, 0, two.alphabet) == (A, 1, H.FINISH_RUNNING, 1)
    # nothing left to draw ranks before the automaton: length, no draw, the state stays
    assert H.sample_dfa(row, 4, 1.0, 1.0, 5, 7, [A], 1, two.table, 1, two.alphabet) == (None, 1, H.FINISH_LENGTH, 1)
    assert H.sample_dfa(row, 4, 1.0, 1.0, 5, 7, [A], 9, two.table, 1, two.alphabet, hist_len=1) == (None, 1, H.FINISH_LENGTH, 1)
    # dead ends draw nothing: a state that permits nothing, one past the table, a negative one, one emptied by the global mask
    dead = np.array([[1, -1, -1, -1, -1, -1, -1, -1], [-1] * 8], dtype=np.int32)
    for table, q, allowed in ((dead, 1, None), (dead, 2, None), (dead, -1, None), (dead, 0, H.allowed_mask(TOK, "CGT")), (dead, 10 ** 9, None)):
        assert H.sample_dfa(row, 4, 1.0, 1.0, 5, 7, [C, C], 9, table, q, ACGT, allowed) == (None, 2, H.FINISH_DEAD_END, q)
    # base < 0: sample_ctl, the state untouched (even a state that would be a dead end)
    allowed = H.allowed_mask(TOK, "ACGT")
    for lim, stop in ((9, ()), (3, ()), (9, set(ACGT))):
        assert H.sample_dfa(row, 4, 1.0, 1.0, 5, 7, [C, C], lim, dead, 1, ACGT, allowed, stop, base=-1) \
            == H.sample_ctl(row, 4, 1.0, 1.0, 5, 7, [C, C], lim, allowed, stop) + (1,)


# ------------------------------------------------------------------------------------------------ C ABI
def test_the_entry_is_exported_and_refuses_before_any_launch():
    header = open(os.path.join(ROOT, "include", "evo_mi355x.h")).read()
    name = "evo_sample_rows_dfa_f32"
    assert name in _build.EXPORTS and name in evo_ops._SIGNATURES and re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert int(re.search(r"#define EVO_ABI_VERSION (\d+)", header).group(1)) == evo_ops.ABI_VERSION >= 18
    assert re.search(r"#define EVO_DFA_ACCEPT \(-2\)", header) and hasattr(evo_ops.HipOps, "sample_rows_dfa")
    lib = evo_ops.load_library()
    assert lib.evo_abi_version() == evo_ops.ABI_VERSION
    f = lib.evo_sample_rows_dfa_f32
    one = ctypes.c_void_p(16)                                         # (non-null, 16-byte aligned, never dereferenced)
    seq, ln = H.pack_stop_sequences([[T, A, A]])                      # host arrays: these ARE read by the entry
    alpha = torch.tensor(ACGT, dtype=torch.int32)
    ctl_names = ["logits", "logits_f32", "ld", "top_k", "top_p", "temperature", "allow", "seed", "stream_id", "count", "active", "ids_out",
                 "logprob_out", "hist_ids", "hist_logits", "hist_logprob", "hist_len", "limit", "stop_mask", "stop_seq", "stop_seq_len", "n_seq",
                 "stop_frame", "length", "finish"]
    names = ctl_names + ["dfa_alphabet", "n_sym", "dfa_next", "n_states", "dfa_base", "dfa_state", "S", "V", "stream"]
    ok = dict(logits=one, logits_f32=0, ld=512, top_k=one, top_p=one, temperature=one, allow=None, seed=1, stream_id=None, count=one,
              active=one, ids_out=one, logprob_out=one, hist_ids=one, hist_logits=None, hist_logprob=None, hist_len=8, limit=one,
              stop_mask=None, stop_seq=seq.data_ptr(), stop_seq_len=ln.data_ptr(), n_seq=1, stop_frame=3, length=one, finish=one,
              dfa_alphabet=alpha.data_ptr(), n_sym=4, dfa_next=one, n_states=3, dfa_base=one, dfa_state=ctypes.c_void_p(4), S=4, V=512,
              stream=None)
    assert list(ok) == names and len(evo_ops._SIGNATURES[name][0]) == len(names)
    # every argument up to `finish` is evo_sample_rows_ctl_f32's, in its order
    assert evo_ops._SIGNATURES[name][0][: len(ctl_names)] == evo_ops._SIGNATURES["evo_sample_rows_ctl_f32"][0][: len(ctl_names)]

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return f(*[a[n] for n in names])
    # what the automaton needs
    for n in ("dfa_alphabet", "dfa_next", "dfa_base", "dfa_state"):
        assert call(**{n: None}) == -1, n
    for n_sym in (0, 9, -1):
        assert call(n_sym=n_sym) == -1, n_sym
    for ids in ([A, C, G, 512], [A, C, G, -1], [A, C, G, A], [A, A, G, T], [1 << 20, C, G, T]):
        bad = torch.tensor(ids, dtype=torch.int32)
        assert call(dfa_alphabet=bad.data_ptr()) == -1, ids
    eight = torch.tensor([0, 7, 8, 504, 511, 65, 66, 65], dtype=torch.int32)            # a duplicate in the last of 8 places
    assert call(dfa_alphabet=eight.data_ptr(), n_sym=8) == -1
    for n_states in (0, -5, (1 << 27) + 1):
        assert call(n_states=n_states) == -1, n_states
    assert call(dfa_next=ctypes.c_void_p(8)) == -1 and call(dfa_next=ctypes.c_void_p(24)) == -1       # 16-byte alignment of the table
    # everything the control entry refuses
    for n in ("count", "active", "limit", "length", "finish", "logits", "top_k", "top_p", "temperature", "ids_out", "logprob_out"):
        assert call(**{n: None}) == -1, n
    assert call(S=0) == -1 and call(V=256) == -1 and call(ld=500) == -1 and call(ld=516) == -1
    assert call(logits=ctypes.c_void_p(8)) == -1 and call(hist_logits=ctypes.c_void_p(24)) == -1
    assert call(hist_len=0) == -1
    assert call(hist_ids=None, n_seq=0, hist_logprob=one, hist_len=0) == -1
    nine = torch.full((9, 8), A, dtype=torch.int32)
    nine_len = torch.full((9,), 3, dtype=torch.int32)
    assert call(stop_seq=nine.data_ptr(), stop_seq_len=nine_len.data_ptr(), n_seq=9) == -1 and call(n_seq=-1) == -1
    for bad in (0, 9, -3):
        bad_len = torch.tensor([bad], dtype=torch.int32)
        assert call(stop_seq_len=bad_len.data_ptr()) == -1, bad
    assert call(hist_ids=None, hist_logprob=one) == -1
    assert call(stop_seq=None) == -1 and call(stop_seq_len=None) == -1
    assert call(stop_frame=0) == -1 and call(stop_frame=-3) == -1


# ------------------------------------------------------------------------------------------------ the scheduler on the oracle backend
class DfaOracleOps(CtlOracleOps):
    """The oracle backend + the automaton launch, row by row from the written specification."""
    dfa_calls = 0

    def sample_rows_dfa(self, logits, top_k, top_p, temperature, seed, count, active, limit, length, finish, dfa_alphabet, dfa_next, dfa_base,
                        dfa_state, stream=None, allow=None, ids_out=None, logprob_out=None, hist_ids=None, hist_logits=None,
                        hist_logprob=None, stop_mask=None, stop_seq=None, stop_frame=1):
        type(self).dfa_calls += 1
        pats = [] if stop_seq is None else [stop_seq[0][q, : int(stop_seq[1][q])].tolist() for q in range(len(stop_seq[1]))]
        table, alphabet = dfa_next.numpy(), dfa_alphabet.tolist()
        for s in range(logits.shape[0]):
            if not bool(active[s]):
                continue
            cnt = int(count[s])
            tok, n, fin, state = H.sample_dfa(logits[s], int(top_k[s]), float(top_p[s]), float(temperature[s]), seed, int(stream[s]),
                                              hist_ids[s, :cnt].tolist(), int(limit[s]), table, int(dfa_state[s]), alphabet, _bits(allow),
                                              _bits(stop_mask), pats, stop_frame, hist_len=hist_ids.shape[1], base=int(dfa_base[s]))
            if tok is not None:
                ids_out.view(-1)[s] = tok
                lp = torch.log_softmax(logits[s].double(), -1)[tok]
                logprob_out[s] = lp
                hist_ids[s, cnt] = tok
                hist_logprob[s, cnt] = lp
                if hist_logits is not None:
                    hist_logits[s, cnt] = logits[s].float()
                count[s] = n
                if int(dfa_base[s]) >= 0:
                    dfa_state[s] = state
            if fin:
                active[s], length[s], finish[s] = False, n, fin


@pytest.fixture(scope="module")
def small():
    from oracle.stripedhyena_ref import RefConfig, make_synthetic_state_dict
    from evo_amd.sh.model import StripedHyena
    sd = make_synthetic_state_dict(RefConfig.from_dict(SMALL), seed=3)
    m = StripedHyena(dict(SMALL), ops=DfaOracleOps(torch.float64))
    m.load_state_dict({k: (v.double() if v.dtype == torch.bfloat16 else v) for k, v in sd.items()})
    return m


SEED, TOP_K, TEMP, N_SPP = 11, 4, 10.0, 2
# one constraint object used by two prompts, two more, two free prompts; unequal limits (the ORF's limit cuts some of its jobs short)
TEMPLATE, PROTEIN, ORF = K.iupac_template("ATGNNRYNTAA"), K.encode_protein("MLS*"), K.open_reading_frame(2)
CONS = [TEMPLATE, None, PROTEIN, ORF, None, TEMPLATE]
LIMITS = [40, 3, 40, 14, 7, 5]
_NAIVE = {}


def naive(m, stop_tokens=None):
    """One job at a time, every token from a full forward of (prompt + tokens so far): [(ids, logprobs, finish)] in job order."""
    key = str(stop_tokens)
    if key in _NAIVE:
        return _NAIVE[key]
    allow = H.allowed_mask(TOK, "ACGT")
    stop = H.allowed_mask(TOK, stop_tokens) if stop_tokens else None
    out = []
    with torch.inference_mode():
        for pi, p in enumerate(PROMPTS):
            c = CONS[pi]
            for k in range(N_SPP):
                hist, lps, fin, state = [], [], 0, 0
                while not fin:
                    row = m(torch.tensor([list(p.encode()) + hist]))[0][0, -1].double()
                    if c is None:
                        tok, n, fin = H.sample_ctl(row, TOP_K, 1.0, TEMP, SEED, pi * N_SPP + k, hist, LIMITS[pi], allow, stop)
                    else:
                        tok, n, fin, state = H.sample_dfa(row, TOP_K, 1.0, TEMP, SEED, pi * N_SPP + k, hist, LIMITS[pi], c.table, state,
                                                          c.alphabet, allow, stop)
                    hist.append(tok)
                    lps.append(float(torch.log_softmax(row, -1)[tok]))
                out.append((hist, lps, fin))
    _NAIVE[key] = out
    return out


def run_pool(m, poll_every=8, **kw):
    gen = {k: kw.pop(k) for k in ("stop_tokens", "return_logits") if k in kw}
    pool = DecodePool(m, TOK, n_slots=3, top_k=TOP_K, top_p=1.0, temperature=TEMP, device="cpu", seed=SEED, allowed_tokens="ACGT",
                      poll_every=poll_every, **kw)
    out = pool.generate(PROMPTS, n_tokens=LIMITS, n_sample_per_prompt=N_SPP, constraints=CONS, **gen)
    return (pool,) + tuple(out)


def check_against_naive(pool, seqs, scores, owner, want):
    assert owner == [pi for pi in range(len(PROMPTS)) for _ in range(N_SPP)]
    assert pool.last_lengths == [len(h) for h, _, _ in want]
    assert pool.last_finish == [H.FINISH_NAMES_ALL[f] for _, _, f in want]
    for j, (hist, lps, fin) in enumerate(want):
        n, c = len(hist), CONS[owner[j]]
        assert pool.last_ids[j, :n].tolist() == hist and (pool.last_ids[j, n:] == -1).all(), j
        # (the tolerance of tests/test_stop_host.py: the oracle sampler stores the fp64 log-probability in f32)
        assert max(abs(x) for x in lps) < 32 and np.allclose(pool.last_logprobs[j, :n].numpy(), lps, rtol=0, atol=2.0 ** -19), j
        assert abs(scores[j] - float(np.mean(lps))) <= 2.0 ** -19
        text = "".join(chr(t) for t in hist)
        assert seqs[j] == (text[:-1] if fin == H.FINISH_STOP_TOKEN else text)          # the accepting token is kept
        if c is not None:                                             # every constrained output is a walk of its automaton
            state = c.walk(hist)
            assert state != K.FORBIDDEN, j
            if fin in (H.FINISH_CONSTRAINT, H.FINISH_LENGTH):         # (a stop token may end a job on its accepting token: reason 1 ranks first)
                assert (state == K.ACCEPT) == (fin == H.FINISH_CONSTRAINT), j


@pytest.mark.parametrize("share", [False, True], ids=["replicated", "shared"])
def test_mixed_constrained_and_free_prompts_equal_the_one_job_loop(small, share):
    want = naive(small)
    runs = [run_pool(small, poll_every=pe, share_prompt_kv=share) for pe in (1, 8)]
    for pool, seqs, scores, owner in runs:
        check_against_naive(pool, seqs, scores, owner, want)
        n_acc = sum(f == H.FINISH_CONSTRAINT for _, _, f in want)
        assert pool.stats["constraint_ends"] == n_acc and pool.stats["length_ends"] == 12 - n_acc and pool.stats["stop_ends"] == 0
        assert pool.stats["polls"] > 0 and pool.stats["tokens"] == sum(pool.last_lengths) - 12
        assert not bool(pool.s_active.any())
        if share:
            assert pool.store_refs == [0] * len(pool.store_refs) and pool.store.row.tolist() == [-1] * 3
    pool, seqs = runs[0][:2]
    # what each kind of job must look like
    for j in (0, 1):
        assert pool.last_finish[j] == "constraint" and re.fullmatch("ATG[ACGT][ACGT][AG][CT][ACGT]TAA", seqs[j]), seqs[j]
    for j in (4, 5):
        assert pool.last_finish[j] == "constraint" and len(seqs[j]) == 12 and "".join(K.GENETIC_CODE[seqs[j][i:i + 3]] for i in (0, 3, 6, 9)) == "MLS*"
    for j in (6, 7):
        assert seqs[j].startswith("ATG") and (pool.last_finish[j] == "constraint") == ORF.accepts(seqs[j])
        assert pool.last_finish[j] == "constraint" or len(seqs[j]) == 14
    for j in (10, 11):
        assert pool.last_finish[j] == "length" and seqs[j] == "ATGNN"[:3] + seqs[j][3:] and len(seqs[j]) == 5
    assert [len(s) for s in seqs[2:4]] == [3, 3] and [len(s) for s in seqs[8:10]] == [7, 7]
    assert pool.last_finish[2:4] == ["length"] * 2 and pool.last_finish[8:10] == ["length"] * 2
    # poll_every changes only the number of reads
    (p1, s1, sc1, _), (p8, s8, sc8, _) = runs
    assert s1 == s8 and sc1 == sc8 and torch.equal(p1.last_ids, p8.last_ids) and torch.equal(p1.last_logprobs, p8.last_logprobs)
    assert torch.equal(p1.last_logits, p8.last_logits) and p1.stats["polls"] >= p8.stats["polls"] and p1.stats["idle_slot_steps"] == 0
    # ONE device table of the distinct automata, a base per prompt
    assert p1.s_dfa_next.shape == (TEMPLATE.n_states + PROTEIN.n_states + ORF.n_states, 8)
    assert np.array_equal(p1.s_dfa_next.numpy(), np.concatenate([TEMPLATE.table, PROTEIN.table, ORF.table]))


def test_other_arguments_stop_rules_and_what_is_refused(small):
    # a stop token beside the constraints: it ends free and constrained jobs alike, ranks before acceptance, and is trimmed
    want = naive(small, "G")
    pool, seqs, scores, owner = run_pool(small, stop_tokens="G", return_logits=False)
    check_against_naive(pool, seqs, scores, owner, want)
    assert "stop_token" in pool.last_finish and all("G" not in s for s in seqs) and pool.last_logits is None
    # one constraint for every prompt; sample_many passes it through; the same pool again replays its table
    calls = DfaOracleOps.dfa_calls
    c = K.iupac_template("ACGTNN")
    _, sm_seqs, sm_scores = sample_many(PROMPTS[:3], small, TOK, n_tokens=9, temp=TEMP, top_k=TOP_K, n_slots=2, device="cpu", seed=SEED,
                                        allowed_tokens="ACGT", constraints=c)
    assert all(re.fullmatch("ACGT[ACGT][ACGT]", s) for s in sm_seqs) and DfaOracleOps.dfa_calls > calls
    p2 = DecodePool(small, TOK, n_slots=2, top_k=TOP_K, temperature=TEMP, device="cpu", seed=SEED, allowed_tokens="ACGT")
    first = p2.generate(PROMPTS[:3], n_tokens=9, constraints=[c, c, c])
    table = p2.s_dfa_next
    assert first[0] == sm_seqs and first[1] == sm_scores and p2.last_finish == ["constraint"] * 3 and p2.stats["constraint_ends"] == 3
    again = p2.generate(PROMPTS[:3], n_tokens=9, constraints=K.iupac_template("TTTTNN"))
    assert p2.s_dfa_next is table and all(s.startswith("TTTT") for s in again[0])      # same size: copied into the table the launch reads
    p2.generate(PROMPTS[:3], n_tokens=9, constraints=K.iupac_template("TTT"))
    assert p2.s_dfa_next is not table
    # without `constraints` the automaton launch is never called
    calls = DfaOracleOps.dfa_calls
    p2.generate(PROMPTS[:3], n_tokens=[2, 3, 4])
    p2.generate(PROMPTS[:3], n_tokens=4, stop_tokens="G")
    p2.generate(PROMPTS[:3], n_tokens=4)
    assert DfaOracleOps.dfa_calls == calls
    # refused before any device work
    mk = lambda **kw: DecodePool(small, TOK, n_slots=2, device="cpu", seed=1, **kw)
    with pytest.raises(ValueError, match="among the allowed"):
        mk(allowed_tokens="ACG").generate(PROMPTS[:1], n_tokens=4, constraints=K.iupac_template("ACT"))
    with pytest.raises(ValueError, match="one alphabet"):
        mk().generate(PROMPTS[:2], n_tokens=4, constraints=[c, K.TokenConstraint([A, C, G], [[-2, -2, -2]])])
    with pytest.raises(ValueError, match="per prompt"):
        mk().generate(PROMPTS[:2], n_tokens=4, constraints=[c])
    with pytest.raises(ValueError, match="per prompt"):
        mk().generate(PROMPTS[:1], n_tokens=4, constraints=["ACGT"])
    with pytest.raises(ValueError, match="permits no token"):
        mk().generate(PROMPTS[:1], n_tokens=4, constraints=K.TokenConstraint(ACGT, [[1, -1, -1, -1], [-1, -1, -1, -1]]))
    plain = DecodePool(small, TOK, n_slots=2, device="cpu", seed=1)
    plain.model = SimpleNamespace(ops=SimpleNamespace(sample_rows_ctl=None), device=torch.device("cpu"))      # a backend without the launch
    with pytest.raises(RuntimeError, match="sample_rows_dfa"):
        plain.generate(PROMPTS[:1], n_tokens=4, constraints=c)
    # a dead end on the device is a bug the host reports: an automaton that skipped validation
    broken = K.TokenConstraint(ACGT, [[1, 1, 1, 1], [-1, -1, -1, -1]])
    broken.validate = lambda allowed=None: broken
    with pytest.raises(RuntimeError, match="permits no token"):
        mk(allowed_tokens="ACGT").generate(PROMPTS[:1], n_tokens=4, constraints=broken)


def test_the_cli_builds_one_constraint_for_all_prompts(tmp_path, monkeypatch):
    """Every flag builds ITS constraint and hands it to DecodePool.generate (a recording pool stands in: no model is loaded)."""
    import evo_amd.pool
    import scripts.sample_many as cli
    calls = []

    class RecordingPool:
        stats = {"steps": 0, "prefills": 0}

        def __init__(self, *a, **kw):
            pass

        def generate(self, prompts, **kw):
            calls.append((list(prompts), kw))
            return [], [], []
    monkeypatch.setattr(evo_amd, "Evo", lambda *a, **kw: SimpleNamespace(model=None, tokenizer=None))
    monkeypatch.setattr(evo_amd.pool, "DecodePool", RecordingPool)
    (tmp_path / "p.txt").write_text("ACGT\nGG\n")
    base = ["--prompts", str(tmp_path / "p.txt"), "--output-csv", str(tmp_path / "out.csv"), "--n-tokens", "30"]

    def built(*flags):
        cli.main(base + list(flags))
        prompts, kw = calls[-1]
        assert prompts == ["ACGT", "GG"] and kw["n_tokens"] == 30
        return kw.get("constraints")

    def same_automaton(c, want):
        return isinstance(c, K.TokenConstraint) and c.alphabet == want.alphabet and np.array_equal(c.table, want.table)
    assert built() is None and "constraints" not in calls[-1][1]                      # without the flags the call is what it was
    assert same_automaton(built("--template", "ATGNNRYTAA"), K.iupac_template("ATGNNRYTAA"))
    assert same_automaton(built("--template", "ATGNNRYTAA", "--then", "free"), K.iupac_template("ATGNNRYTAA", then="free"))
    assert same_automaton(built("--encode-protein", "MKLS*"), K.encode_protein("MKLS*"))
    assert same_automaton(built("--encode-protein", "MK", "--then", "free"), K.encode_protein("MK", then="free"))
    assert same_automaton(built("--orf-min-codons", "7"), K.open_reading_frame(7))
    n = len(calls)
    for bad in (["--template", "ACGT", "--encode-protein", "MK"], ["--template", "ACGT", "--orf-min-codons", "3"],
                ["--orf-min-codons", "3", "--then", "free"], ["--then", "free"], ["--template", "ACGT", "--then", "stop"]):
        with pytest.raises(SystemExit):                               # argparse refuses before anything is built
            cli.main(base + bad)
    assert len(calls) == n


# ------------------------------------------------------------------------------------------------ resources
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_automaton_kernel_needs_no_scratch_and_no_more_lds():
    meta = _metadata("sample.hip")
    old = [v for k, v in meta.items() if "sample_rows_kernel" in k]
    new = [v for k, v in meta.items() if "sample_rows_dfa_kernel" in k]
    assert len(old) == 1 and len(new) == 1, sorted(meta)
    print("sample_rows_kernel", old[0], "sample_rows_dfa_kernel", new[0])
    for r in old + new:
        assert r["scratch"] == 0 and r["spill"] == 0 and r["sgpr_spill"] == 0, r
    assert new[0]["lds"] == old[0]["lds"]                             # alphabet and patterns are launch arguments, the table row registers
