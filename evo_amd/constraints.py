"""Constrained generation for the decode pool: small deterministic automata over a handful of tokens.

A `TokenConstraint` is an alphabet of at most 8 token ids and a table [n_states, 8] of int32: table[q][a] is what drawing alphabet[a] in
state q does -- a next state (>= 0), ACCEPT (-2: the constraint is complete, the job ends with this token) or FORBIDDEN (-1).  State 0
is initial.  The sampler launch `evo_sample_rows_dfa_f32` reads one row of that table per draw and moves the state on the device
(`DecodePool.generate(constraints=...)`); everything here is host-side numpy that builds and checks such tables:

    iupac_template("ATGNNNNNNRRYNNNTAA")          fixed motifs with free stretches, in IUPAC nucleotide codes
    encode_protein("MKLS*")                       any DNA that encodes the protein: synonymous codons are the model's choice
    open_reading_frame(min_codons=50)             ATG, no in-frame stop codon before codon `min_codons`, then the first one ends it
    concat(c1, c2)                                c1, then c2

The genetic code is the standard one (NCBI translation table 1), written out below in the usual TCAG order."""
from __future__ import annotations

from collections import deque
from itertools import product
from typing import Callable, Dict, Hashable, Iterable, List, Optional, Sequence, Tuple, Union

import numpy as np

ACCEPT = -2
FORBIDDEN = -1
MAX_SYMBOLS = 8
VOCAB_BITS = 512
DNA = "ACGT"

IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC", "B": "CGT", "D": "AGT",
         "H": "ACT", "V": "ACG", "N": "ACGT"}

# NCBI translation table 1: the amino acid of codon b1 b2 b3 at index 16 i1 + 4 i2 + i3, every base indexed in the order T C A G
_BASES_TCAG = "TCAG"
_AMINO_ACIDS = "FFLLSSSSYY**CC*WLLLLPPPPHHQQRRRRIIIMTTTTNNKKSSRRVVVVAAAADDEEGGGG"
GENETIC_CODE: Dict[str, str] = {"".join(c): _AMINO_ACIDS[i] for i, c in enumerate(product(_BASES_TCAG, repeat=3))}


def codons_of(residue: str) -> List[str]:
    """The codons of one residue letter (`*`: the stop codons), in TCAG order.  An unknown letter is a ValueError."""
    out = [c for c, aa in GENETIC_CODE.items() if aa == residue]
    if len(residue) != 1 or not out:
        raise ValueError(f"encode_protein: unknown residue {residue!r}")
    return out


def _allowed_ids(allowed) -> Optional[set]:
    """None, a string (its bytes, as the character-level tokenizer reads it), 512 flags, or token ids -> a set of ids (None: all)."""
    if allowed is None:
        return None
    if isinstance(allowed, str):
        return set(allowed.encode())
    arr = np.asarray(allowed)
    if arr.dtype == np.bool_:
        return set(np.nonzero(arr.reshape(-1))[0].tolist())
    return {int(t) for t in arr.reshape(-1).tolist()}


class TokenConstraint:
    """`alphabet`: 1 to 8 distinct token ids in [0, 512); `table`: int32 [n_states, 8] (columns beyond the alphabet are FORBIDDEN)."""

    def __init__(self, alphabet: Sequence[int], table):
        self.alphabet: Tuple[int, ...] = tuple(int(t) for t in alphabet)
        if not 1 <= len(self.alphabet) <= MAX_SYMBOLS or len(set(self.alphabet)) != len(self.alphabet):
            raise ValueError(f"TokenConstraint: an alphabet has 1 to {MAX_SYMBOLS} distinct token ids")
        if any(not 0 <= t < VOCAB_BITS for t in self.alphabet):
            raise ValueError(f"TokenConstraint: a token id of {self.alphabet} is outside [0, {VOCAB_BITS})")
        t = np.asarray(table)
        if t.ndim != 2 or t.shape[0] < 1 or not len(self.alphabet) <= t.shape[1] <= MAX_SYMBOLS or not np.issubdtype(t.dtype, np.integer):
            raise ValueError("TokenConstraint: the table is an integer matrix [n_states >= 1, len(alphabet) ... 8]")
        self.table = np.full((t.shape[0], MAX_SYMBOLS), FORBIDDEN, dtype=np.int32)
        self.table[:, : len(self.alphabet)] = t[:, : len(self.alphabet)]
        self._check_transitions()                                     # (so that walk / min_length never index past the table)

    @property
    def n_states(self) -> int:
        return int(self.table.shape[0])

    def __repr__(self) -> str:
        return f"TokenConstraint(alphabet={self.alphabet}, n_states={self.n_states})"

    def _symbols(self, ids) -> List[int]:
        """Token ids (or a string: its bytes) -> symbol indices, -1 for a token outside the alphabet."""
        ids = list(ids.encode()) if isinstance(ids, str) else [int(t) for t in ids]
        index = {t: a for a, t in enumerate(self.alphabet)}
        return [index.get(t, -1) for t in ids]

    def _permitted(self, q: int, allowed: Optional[set]) -> List[int]:
        return [a for a, t in enumerate(self.alphabet)
                if (self.table[q, a] >= 0 or self.table[q, a] == ACCEPT) and (allowed is None or t in allowed)]

    def walk(self, ids) -> int:
        """The state after the tokens `ids` from state 0: >= 0, ACCEPT when the last token took an ACCEPT edge, FORBIDDEN when a token
        was not permitted where it stood (or followed an ACCEPT edge: the job is over there)."""
        q = 0
        for a in self._symbols(ids):
            if q < 0 or a < 0:
                return FORBIDDEN
            q = int(self.table[q, a])
            if q < 0 and q != ACCEPT:
                return FORBIDDEN
        return q

    def accepts(self, ids) -> bool:
        return self.walk(ids) == ACCEPT

    def _check_transitions(self) -> None:
        n = self.n_states
        live = self.table[:, : len(self.alphabet)]
        bad = (live >= n) | ((live < 0) & (live != ACCEPT) & (live != FORBIDDEN))
        if bool(bad.any()):
            q, a = (int(v[0]) for v in np.nonzero(bad))
            raise ValueError(f"TokenConstraint: transition {int(live[q, a])} of state {q} is outside [0, {n}) and neither ACCEPT nor FORBIDDEN")

    def validate(self, allowed=None) -> "TokenConstraint":
        """ValueError for a transition that is neither a state of the table, ACCEPT nor FORBIDDEN (the constructor refuses one too; `table`
        can be written to afterwards), and for a state reachable from 0 -- through tokens that `allowed` (see `_allowed_ids`) permits -- in
        which no permitted token is left: a job there could not go on."""
        self._check_transitions()
        ok = _allowed_ids(allowed)
        seen, todo = {0}, deque([0])
        while todo:
            q = todo.popleft()
            steps = self._permitted(q, ok)
            if not steps:
                raise ValueError(f"TokenConstraint: state {q} can be reached and permits no token" + ("" if ok is None else " among the allowed ones"))
            for a in steps:
                nxt = int(self.table[q, a])
                if nxt >= 0 and nxt not in seen:
                    seen.add(nxt)
                    todo.append(nxt)
        return self

    def min_length(self) -> Optional[int]:
        """The fewest tokens that complete the constraint; None when no path from state 0 reaches ACCEPT."""
        dist, todo = {0: 0}, deque([0])
        while todo:
            q = todo.popleft()
            for a in self._permitted(q, None):
                nxt = int(self.table[q, a])
                if nxt == ACCEPT:
                    return dist[q] + 1
                if nxt not in dist:
                    dist[nxt] = dist[q] + 1
                    todo.append(nxt)
        return None


def _build(alphabet: str, start: Hashable, step: Callable[[Hashable, str], Union[Hashable, int, None]]) -> TokenConstraint:
    """Numbers the states reachable from `start` breadth first.  step(state, letter) -> the next state (any hashable key that is not an
    int), ACCEPT, or None (forbidden)."""
    index, rows, todo = {start: 0}, [], deque([start])
    while todo:
        key = todo.popleft()
        row = [FORBIDDEN] * MAX_SYMBOLS
        for a, letter in enumerate(alphabet):
            nxt = step(key, letter)
            if nxt is None:
                continue
            if nxt == ACCEPT and isinstance(nxt, int):
                row[a] = ACCEPT
                continue
            if nxt not in index:
                index[nxt] = len(index)
                todo.append(nxt)
            row[a] = index[nxt]
        rows.append(row)
    return TokenConstraint([ord(c) for c in alphabet], np.array(rows, dtype=np.int32))


_FREE = ("free",)                                                      # the state behind a constraint built with then="free": loops on everything


def _after(then: str):
    if then not in ("end", "free"):
        raise ValueError('then: "end" (the job ends with the constraint) or "free" (it goes on unconstrained)')
    return ACCEPT if then == "end" else _FREE


def iupac_template(template: str, then: str = "end") -> TokenConstraint:
    """Position i permits the nucleotides of the IUPAC code template[i] (A C G T R Y S W K M B D H V N)."""
    done = _after(then)
    sets = []
    for c in template:
        if c not in IUPAC:
            raise ValueError(f"iupac_template: {c!r} is not an IUPAC nucleotide code")
        sets.append(IUPAC[c])
    if not sets:
        raise ValueError("iupac_template: the template is empty")

    def step(key, letter):
        if key == _FREE:
            return _FREE
        if letter not in sets[key[1]]:
            return None
        return ("at", key[1] + 1) if key[1] + 1 < len(sets) else done
    return _build(DNA, ("at", 0), step)


def encode_protein(protein: str, then: str = "end") -> TokenConstraint:
    """Any DNA whose codons translate to `protein` (one-letter residues of the standard genetic code, `*` = any stop codon).  Per residue:
    a root, the first letters that start one of its codons, their two-letter prefixes -- at most 21 states."""
    done = _after(then)
    codons = [codons_of(r) for r in protein]
    if not codons:
        raise ValueError("encode_protein: the protein is empty")

    def step(key, letter):
        if key == _FREE:
            return _FREE
        i, prefix = key
        prefix += letter
        if not any(c.startswith(prefix) for c in codons[i]):
            return None
        if len(prefix) < 3:
            return (i, prefix)
        return (i + 1, "") if i + 1 < len(codons) else done
    return _build(DNA, (0, ""), step)


def open_reading_frame(min_codons: int, start: Optional[str] = "ATG", stops: Iterable[str] = ("TAA", "TAG", "TGA")) -> TokenConstraint:
    """`start` (forced when given; it is codon 1), then codons: a stop codon cannot be completed as a codon before codon number
    `min_codons` -- the edge that would complete it is forbidden -- and ends the job (ACCEPT) from there on."""
    min_codons, stops = int(min_codons), [str(s) for s in stops]
    if min_codons < 1:
        raise ValueError("open_reading_frame: min_codons must be >= 1")
    if not stops or any(len(s) != 3 or set(s) - set(DNA) for s in stops):
        raise ValueError("open_reading_frame: stop codons are three letters of ACGT")
    if start is not None and (len(start) != 3 or set(start) - set(DNA) or start in stops):
        raise ValueError("open_reading_frame: the start codon is three letters of ACGT and no stop codon")
    prefixes = {s[:k] for s in stops for k in (1, 2)}

    # key = ("start", letters of the start codon emitted) | (codons completed, capped at min_codons - 1, position in the codon,
    #        the letters of the codon so far while they are still the prefix of a stop codon, else None)
    def step(key, letter):
        if key[0] == "start":
            if letter != start[key[1]]:
                return None
            return ("start", key[1] + 1) if key[1] < 2 else (min(1, min_codons - 1), 0, "")
        done, pos, prefix = key
        word = None if prefix is None else prefix + letter
        if pos < 2:
            return (done, pos + 1, word if word in prefixes else None)
        if word in stops:
            return ACCEPT if done + 1 >= min_codons else None
        return (min(done + 1, min_codons - 1), 0, "")
    return _build(DNA, ("start", 0) if start is not None else (0, 0, ""), step)


def concat(c1: TokenConstraint, c2: TokenConstraint) -> TokenConstraint:
    """c1, then c2: c1's ACCEPT edges lead to c2's state 0, c2's states follow c1's."""
    if c1.alphabet != c2.alphabet:
        raise ValueError("concat: the two constraints must have the same alphabet")
    n1 = c1.n_states
    first = np.where(c1.table == ACCEPT, np.int32(n1), c1.table)
    second = np.where(c2.table >= 0, c2.table + np.int32(n1), c2.table)
    return TokenConstraint(c1.alphabet, np.concatenate([first, second]).astype(np.int32))
