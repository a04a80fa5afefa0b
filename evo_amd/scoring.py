"""Scoring entry points with the reference's signatures [REF evo/scoring.py:9-131].

Differences from the reference, all host-side and documented in DESIGN.md:
  * `prepare_batch` assembles the padded id matrix on the host and does ONE host->device copy (the
    reference copies every sequence separately [REF evo/scoring.py:23-31]); the ids are identical.
  * log-softmax / entropy run in fp32 inside one gfx950 kernel (`evo_logprob_entropy`) instead of a
    bf16 `torch.log_softmax` [REF evo/scoring.py:47,119] -- the reference rounds log-probs to 3
    significant digits; pass `bf16_logprobs=True` to reproduce that rounding.
  * `position_profiles` / `substitution_scores` (no counterpart in the reference): per position, the log-probability of
    chosen tokens (A, C, G, T) next to the observed token's log-prob and the entropy, from ONE forward whose tail is one
    launch of `evo_unembed_profile_bf16` -- the [B, T, 512] logits are never materialised.
"""
from typing import List, NamedTuple, Sequence, Tuple, Union

import numpy as np
import torch

from .backend import Backend
from .tokenizer import CharLevelTokenizer


def prepare_batch(seqs: List[str], tokenizer: CharLevelTokenizer, prepend_bos: bool = True,
                  device: str = "cuda:0") -> Tuple[torch.Tensor, List[int]]:
    """Tokenise, (optionally) prepend BOS = eod_id, right-pad with pad_id to the longest sequence.
    Returns (input_ids [B, T] int64 on `device`, list of sequence lengths)."""
    seq_lengths = [len(s) for s in seqs]
    longest = max(seq_lengths)
    bos = int(prepend_bos)
    rows = [np.frombuffer(seq.encode(), dtype=np.uint8) for seq in seqs]
    # every row is  BOS? + bytes + (longest - len(seq)) pads; with non-ASCII text the byte count differs
    # from the character count and rows stop lining up -- the reference's torch.cat raises there too
    widths = {bos + r.size + (longest - n) for r, n in zip(rows, seq_lengths)}
    if len(widths) != 1:
        raise RuntimeError("prepare_batch: rows have different token lengths (non-ASCII input?)")
    width = widths.pop()
    ids = np.full((len(seqs), width), tokenizer.pad_id, dtype=np.int64)
    if prepend_bos:
        ids[:, 0] = tokenizer.eod_id
    for i, r in enumerate(rows):
        ids[i, bos:bos + r.size] = r
    return torch.from_numpy(ids).to(device), seq_lengths


def _ops_for(t: torch.Tensor):
    from .ops import default_ops
    return default_ops()


def logits_to_logprobs(logits: torch.Tensor, input_ids: torch.Tensor, trim_bos: bool = True,
                       bf16_logprobs: bool = False) -> torch.Tensor:
    """(batch, length, vocab) logits -> (batch, length) log-likelihood of each provided token.
    With trim_bos the last prediction and the first (BOS) id are dropped so position t scores token t+1."""
    if trim_bos:
        logits = logits[:, :-1]
        input_ids = input_ids[:, 1:]
    assert logits.shape[1] == input_ids.shape[1]
    B, L, V = logits.shape
    if logits.is_cuda:
        lg = logits.reshape(B * L, V)
        if lg.dtype not in (torch.bfloat16, torch.float32):
            lg = lg.float()
        lp, _ = _ops_for(lg).logprob_entropy(lg.contiguous(), input_ids.reshape(-1).to(lg.device))
        out = lp.view(B, L)
    else:   # host tensors (utility use only; the scoring hot path always hands over device logits)
        out = torch.log_softmax(logits.float(), dim=-1).gather(2, input_ids.unsqueeze(-1).long()).squeeze(-1)
    return out.to(torch.bfloat16) if bf16_logprobs else out


def _fused_tail_ok(model, input_ids) -> bool:
    """The fused unembed + log-softmax + gather kernel serves the engine's own model class on the GPU."""
    ops = getattr(model, "ops", None) if hasattr(model, "hidden_states") else None
    if not getattr(model, "has_own_unembed", True) or not isinstance(getattr(getattr(model, "unembed", None), "weight", None), torch.Tensor):
        return False                    # model.unembed replaced (e.g. by an identity module): model(ids) returns what it makes
    return (isinstance(ops, Backend) and ops.name == "hip-gfx950" and ops.supports("unembed_logprob")
            and ops.unembed_logprob_ok(model.unembed.weight.new_empty(1, model.hidden_size), model.unembed.weight))


def score_logprobs_device(model, input_ids: torch.Tensor, want_entropy: bool = False):
    """What `score_sequences` / `positional_entropies` compute on the device for a BOS-prefixed id matrix [B, T]:
    (log-prob of token t+1 at position t  [B, T-1] f32 | None, entropy of the next-token distribution [B, T-1] f32 |
    None).  On the MI355X engine the unembedding, the log-softmax and the gather run as ONE kernel
    (evo_unembed_logprob_bf16) and the [B, T, 512] logits are never materialised; any other model object takes
    model(ids) -> logits_to_logprobs like the reference [REF evo/scoring.py:80-84,116-121]."""
    B, T = input_ids.shape
    if _fused_tail_ok(model, input_ids):
        with torch.no_grad():
            hid = model.hidden_states(input_ids)                       # [B*T, D] final-norm output
            tgt = torch.full((B, T), -1, dtype=torch.int64, device=hid.device)
            tgt[:, :-1] = input_ids[:, 1:].to(hid.device)
            lp, en = model.ops.unembed_logprob(hid, model.unembed.weight, tgt.reshape(-1),
                                               want_logprob=not want_entropy, want_entropy=want_entropy)
        return (None if lp is None else lp.view(B, T)[:, :-1]), (None if en is None else en.view(B, T)[:, :-1])
    logits, _ = model(input_ids)
    if not want_entropy:
        return logits_to_logprobs(logits, input_ids, trim_bos=True), None
    logits = logits[:, :-1]                                            # BOS was prepended: drop the last prediction
    L, V = logits.shape[1], logits.shape[2]
    if logits.is_cuda:
        lg = logits.reshape(B * L, V).contiguous()
        _, ent = _ops_for(lg).logprob_entropy(lg, None, want_logprob=False, want_entropy=True)
        return None, ent.view(B, L)
    lsm = torch.log_softmax(logits.float(), dim=-1)
    return None, -(lsm.exp() * lsm).sum(-1)


def _reduce(logprobs: np.ndarray, seq_lengths: List[int], reduce_method: str) -> List[float]:
    if reduce_method == "mean":
        fn = np.mean
    elif reduce_method == "sum":
        fn = np.sum
    else:
        raise ValueError(f"Invalid reduce_method {reduce_method}")
    return [fn(logprobs[i][: seq_lengths[i]]) for i in range(len(seq_lengths))]


def score_sequences(seqs: List[str], model, tokenizer: CharLevelTokenizer, reduce_method: str = "mean",
                    device: str = "cuda:0") -> List[float]:
    """Mean (or sum) per-token log-likelihood of each sequence under the model."""
    if reduce_method not in ("mean", "sum"):
        raise ValueError(f"Invalid reduce_method {reduce_method}")
    input_ids, seq_lengths = prepare_batch(seqs, tokenizer, device=device, prepend_bos=True)
    assert len(seq_lengths) == input_ids.shape[0]
    with torch.inference_mode():
        logprobs, _ = score_logprobs_device(model, input_ids)          # (batch, length - 1)
    return _reduce(logprobs.float().cpu().numpy(), seq_lengths, reduce_method)


def positional_entropies(seqs: List[str], model, tokenizer: CharLevelTokenizer,
                         device: str = "cuda:0") -> List[np.ndarray]:
    """Per-position entropy of the next-token distribution, one array (len(seq)) per sequence."""
    input_ids, seq_lengths = prepare_batch(seqs, tokenizer, device=device, prepend_bos=True)
    assert len(seq_lengths) == input_ids.shape[0]
    with torch.inference_mode():
        _, ent = score_logprobs_device(model, input_ids, want_entropy=True)
    ent = ent.float().cpu().numpy()
    out = [ent[i][: seq_lengths[i]] for i in range(len(seq_lengths))]
    assert all(len(s) == len(e) for s, e in zip(seqs, out))
    return out


# ---- per-position profiles: what the model thinks of A, C, G and T at every position ---------------------------------------
PROFILE_MAX_TOKENS = 8      # ids one launch of the fused tail's profile epilogue takes (HipOps.PROFILE_MAX_IDS)


class PositionProfile(NamedTuple):
    """One sequence's record of `position_profiles`; index i is the model's distribution of seq[i] given seq[:i]."""
    logprob: np.ndarray             # [L] f32: log-prob of the observed token seq[i]
    entropy: np.ndarray             # [L] f32: entropy of the distribution at position i
    token_logprobs: np.ndarray      # [L, n] f32: log-prob of each token of `tokens` at position i
    tokens: Tuple[int, ...]         # the n token ids, in column order


def profile_token_ids(tokens: Union[str, Sequence[int]] = "ACGT", vocab: int = 512) -> Tuple[int, ...]:
    """`tokens` as a tuple of 1 .. 8 distinct ids in [0, vocab): an ASCII string (each character is its byte id, as the
    byte-level tokenizer maps it) or a sequence of ints.  Anything else is a ValueError -- raised before any device work."""
    if isinstance(tokens, (str, bytes)):
        raw = tokens.encode("utf-8") if isinstance(tokens, str) else tokens
        if isinstance(tokens, str) and len(raw) != len(tokens):
            raise ValueError(f"tokens: {tokens!r} holds a non-ASCII character (one character must be one byte id)")
        ids = list(raw)
    else:
        if isinstance(tokens, torch.Tensor):
            tokens = tokens.tolist()
        try:
            tokens = list(tokens)
            ids = [int(t) for t in tokens]
        except (TypeError, ValueError) as e:
            raise ValueError(f"tokens: expected an ASCII string or a sequence of ints, got {tokens!r}") from e
        if any(i != t for i, t in zip(ids, tokens)):
            raise ValueError(f"tokens: expected integer ids, got {tokens!r}")
    if not 1 <= len(ids) <= PROFILE_MAX_TOKENS:
        raise ValueError(f"tokens: expected 1 to {PROFILE_MAX_TOKENS} tokens, got {len(ids)}")
    for i in ids:
        if not 0 <= i < vocab:
            raise ValueError(f"tokens: id {i} is outside [0, {vocab})")
    if len(set(ids)) != len(ids):
        raise ValueError(f"tokens: a token is given twice in {tokens!r}")
    return tuple(ids)


def score_profile_device(model, input_ids: torch.Tensor, token_ids):
    """For a BOS-prefixed id matrix [B, T]: (log-prob of token t+1 at position t [B, T-1] f32, entropy of the next-token
    distribution [B, T-1] f32, log-prob of every token of `token_ids` at position t [B, T-1, n] f32), on the device.  On the
    MI355X engine: model.hidden_states, then ONE launch of evo_unembed_profile_bf16 -- the first two are bit for bit what
    `score_logprobs_device` returns, and the [B, T, 512] logits are never materialised.  Any other model object (and
    EVO_AMD_FUSED_TAIL=0) takes model(ids) -> an fp32 log-softmax where the logits live -> gather / index_select."""
    ids = profile_token_ids(token_ids)
    B, T = input_ids.shape
    if _fused_tail_ok(model, input_ids) and model.ops.supports("unembed_profile"):
        with torch.no_grad():
            hid = model.hidden_states(input_ids)                       # [B*T, D] final-norm output
            tgt = torch.full((B, T), -1, dtype=torch.int64, device=hid.device)
            tgt[:, :-1] = input_ids[:, 1:].to(hid.device)
            sl, lp, en = model.ops.unembed_profile(hid, model.unembed.weight, ids, tgt.reshape(-1))
        return lp.view(B, T)[:, :-1], en.view(B, T)[:, :-1], sl.view(B, T, len(ids))[:, :-1]
    with torch.no_grad():
        logits, _ = model(input_ids)
        lsm = torch.log_softmax(logits[:, :-1].float(), dim=-1)       # BOS was prepended: drop the last prediction
        lp = lsm.gather(2, input_ids[:, 1:].to(lsm.device).unsqueeze(-1).long()).squeeze(-1)
        en = -(lsm.exp() * lsm).sum(-1)
        sl = lsm.index_select(2, torch.tensor(ids, dtype=torch.int64, device=lsm.device))
    return lp, en, sl


def position_profiles(seqs: List[str], model, tokenizer: CharLevelTokenizer, tokens: Union[str, Sequence[int]] = "ACGT",
                      device: str = "cuda:0") -> List[PositionProfile]:
    """Per position of every sequence: the log-prob of the observed token, the entropy, and the log-probs of `tokens`
    (an ASCII string or 1 .. 8 distinct ids in [0, 512)) -- one `PositionProfile` per sequence, trimmed to len(seq), from ONE
    forward.  The convention is the reference's scoring one [REF evo/scoring.py:47-57]: index i holds the distribution of
    seq[i] given seq[:i].  From a record `p`:
      substitution_scores(p)                       log-likelihood ratio of every alternative against the observed token
      p.token_logprobs.argmax(-1)                  the predicted token's column (predicted_tokens(p): its id)
      renormalized(p)                              the distribution over `tokens` alone (log-softmax over the columns)"""
    ids = profile_token_ids(tokens)                                    # ValueError before any device work
    if len(seqs) == 0:
        raise ValueError("position_profiles: no sequences")
    input_ids, seq_lengths = prepare_batch(seqs, tokenizer, device=device, prepend_bos=True)
    with torch.inference_mode():
        lp, en, sl = score_profile_device(model, input_ids, ids)
    lp, en, sl = lp.float().cpu().numpy(), en.float().cpu().numpy(), sl.float().cpu().numpy()
    out = [PositionProfile(lp[i][:n].copy(), en[i][:n].copy(), sl[i][:n].copy(), ids) for i, n in enumerate(seq_lengths)]
    assert all(len(s) == len(p.logprob) for s, p in zip(seqs, out))
    return out


def substitution_scores(profile: PositionProfile) -> np.ndarray:
    """[L, n]: token_logprobs - logprob[:, None], the log-likelihood ratio of each alternative token against the observed one
    at every position (exactly 0 where the alternative IS the observed token).  This is the FIRST-ORDER variant-effect score:
    it is conditioned on the prefix only.  What a substitution does to the likelihood of the SUFFIX is `score_variants` below
    (`single_substitutions` enumerates the scan)."""
    return profile.token_logprobs - profile.logprob[:, None]


def predicted_tokens(profile: PositionProfile) -> np.ndarray:
    """[L] int64: at every position the id, among `profile.tokens`, the model gives the highest probability."""
    return np.asarray(profile.tokens, dtype=np.int64)[profile.token_logprobs.argmax(-1)]


def renormalized(profile: PositionProfile) -> np.ndarray:
    """[L, n]: log-probs renormalised over `profile.tokens` alone (a log-softmax over the columns, in fp64 -> f32)."""
    x = profile.token_logprobs.astype(np.float64)
    m = x.max(-1, keepdims=True)
    return (x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))).astype(np.float32)


# ---- variants of one reference: which prefix each one shares with it ----------------------------------------------------------------
VARIANT_MIN_SUFFIX = 129     # rows a variant's suffix needs for HipOps.attention_prefix (csrc/attn_w64.hip SEG: only the 64-rows-per-wave form is built)


class VariantGroup(NamedTuple):
    """One pass of `plan_variants`: the variants `index` (positions in the caller's list) resume from `checkpoint` tokens of the
    reference (0: an ordinary stateless forward); a pass forwards `rows` rows -- the reference's own suffix first -- of `width` tokens."""
    checkpoint: int
    index: Tuple[int, ...]
    rows: int
    width: int


class VariantPlan(NamedTuple):
    first_diff: np.ndarray          # [N] int64: first index at which the variant's ids differ from the reference's; -1 = equal
    checkpoint: np.ndarray          # [N] int64: tokens of the reference the variant resumes from (-1 for a copy of the reference)
    groups: Tuple[VariantGroup, ...]
    checkpoints: Tuple[int, ...]    # the checkpoints > 0 in use, ascending: where the reference pass keeps a snapshot
    tokens: int                     # tokens forwarded: the reference once + rows * width of every pass
    naive_tokens: int               # what one full forward per variant (and the reference) forwards, padded to the longest


def first_difference(ref_ids: Sequence[int], var_ids: Sequence[int]) -> int:
    """First index at which two id sequences differ; the shorter length when one is a prefix of the other; -1 when equal."""
    n = min(len(ref_ids), len(var_ids))
    a, b = np.asarray(ref_ids[:n]), np.asarray(var_ids[:n])
    ne = np.nonzero(a != b)[0]
    if ne.size:
        return int(ne[0])
    return -1 if len(ref_ids) == len(var_ids) else n


def plan_variants(ref_ids: Sequence[int], variant_ids: Sequence[Sequence[int]], checkpoint_every: int = 512,
                  max_batch_tokens: int = 65536, max_rows_per_pass: int = 64, cached: bool = True) -> VariantPlan:
    """Pure host planning of variant scoring from cached prefixes of one reference.  ids are BOS + tokens.

    With lp[t] = log p(ids[t+1] | ids[:t+1]) and d the first index at which a variant's ids differ from the reference's, position
    d - 1 is the first whose log-prob changes (it predicts the changed token).  The variant resumes from checkpoint c = the largest
    multiple of `checkpoint_every` with c <= d - 1 and T_v - c >= VARIANT_MIN_SUFFIX (the shared-prefix attention kernel's shortest
    query range).  If none qualifies, c = 0: an ordinary forward.
    Variants are grouped by c.  Within a checkpoint they are cut into passes of at most `max_batch_tokens` (rows x padded suffix
    length, the reference's own suffix row included) and never more than `max_rows_per_pass` rows.
    `tokens` counts a separate pass over the reference only when a checkpoint > 0 is in use (or when there is no pass at all);
    otherwise the reference's log-probs come from row 0 of a stateless pass.  cached=False (a model without the cache path): every
    variant gets c = 0."""
    if checkpoint_every <= 0 or checkpoint_every % 64:
        raise ValueError(f"checkpoint_every must be a positive multiple of 64 (whole key tiles of the shared prefix), got {checkpoint_every}")
    if max_rows_per_pass < 2 or max_batch_tokens < 1:
        raise ValueError("a pass needs room for the reference's row and one variant")
    Tr = len(ref_ids)
    N = len(variant_ids)
    d = np.array([first_difference(ref_ids, v) for v in variant_ids], dtype=np.int64).reshape(N)
    ck = np.full(N, -1, dtype=np.int64)
    for n, v in enumerate(variant_ids):
        if d[n] < 0:
            continue
        c = max(int(d[n]) - 1, 0) // checkpoint_every * checkpoint_every if cached else 0
        while c > 0 and len(v) - c < VARIANT_MIN_SUFFIX:
            c -= checkpoint_every
        ck[n] = max(c, 0)
    groups = []
    for c in sorted(set(int(x) for x in ck if x >= 0)):
        members = [n for n in range(N) if ck[n] == c]
        cur = []

        def width(idx):
            return max([Tr - c] + [len(variant_ids[n]) - c for n in idx])

        def flush():
            if cur:
                groups.append(VariantGroup(c, tuple(cur), len(cur) + 1, width(cur)))
        for n in members:
            if cur and (len(cur) + 2 > max_rows_per_pass or (len(cur) + 2) * width(cur + [n]) > max_batch_tokens):
                flush()
                cur = []
            cur.append(n)
        flush()
    tokens = sum(g.rows * g.width for g in groups)
    if not groups or any(g.checkpoint > 0 for g in groups):
        tokens += Tr                                                   # the reference on its own: the cached pass, or nothing else to run
    longest = max([Tr] + [len(v) for v in variant_ids])
    return VariantPlan(d, ck, tuple(groups), tuple(sorted({g.checkpoint for g in groups if g.checkpoint > 0})), int(tokens),
                       int((N + 1) * longest))


def single_substitutions(seq: str, positions=None, alphabet: str = "ACGT"):
    """Every single substitution of `seq` at `positions` (default: all; 0-based nucleotide indices) by another letter of `alphabet`,
    as a list of (position, alt, sequence) in position order, the alphabet's order within a position."""
    positions = range(len(seq)) if positions is None else [int(p) for p in positions]
    out = []
    for p in positions:
        if not 0 <= p < len(seq):
            raise ValueError(f"single_substitutions: position {p} is outside the sequence (length {len(seq)})")
        for alt in alphabet:
            if alt != seq[p]:
                out.append((p, alt, seq[:p] + alt + seq[p + 1:]))
    return out


class VariantScores(NamedTuple):
    score: np.ndarray               # [N] f64: what score_sequences(variants, reduce_method) returns
    delta: np.ndarray               # [N] f64: summed log-likelihood of the variant minus the reference's (independent of reduce_method)
    first_diff: np.ndarray          # [N] int64: VariantPlan.first_diff
    reference_score: float
    stats: dict                     # tokens forwarded, passes, checkpoints used, the naive token count


def _bos_ids(seq: str, tokenizer) -> np.ndarray:
    raw = np.frombuffer(seq.encode(), dtype=np.uint8).astype(np.int64)
    if raw.size != len(seq):
        raise RuntimeError("score_variants: non-ASCII input")
    return np.concatenate([[tokenizer.eod_id], raw])


def _logprobs_of(model, ids: torch.Tensor, tgt: torch.Tensor, cache=None) -> np.ndarray:
    """[B, T] f64 host array: log p(tgt[b, t] | ids[b, :t+1]) (0 where tgt < 0), through the cache when one is given."""
    B, T = ids.shape
    with torch.no_grad():
        if hasattr(model, "hidden_states"):
            hid = model.hidden_states(ids, cache)
            if _fused_tail_ok(model, ids):
                lp, _ = model.ops.unembed_logprob(hid, model.unembed.weight, tgt.reshape(-1).to(hid.device))
                return lp.view(B, T).double().cpu().numpy()
            logits = model.unembed.unembed(hid).view(B, T, -1)
        else:
            logits = model(ids)[0]
        lsm = torch.log_softmax(logits if logits.dtype == torch.float64 else logits.float(), dim=-1)
        t = tgt.to(lsm.device)
        lp = lsm.gather(2, t.clamp(min=0).unsqueeze(-1)).squeeze(-1).masked_fill(t < 0, 0.0)
    return lp.double().cpu().numpy()


def _padded(rows: List[np.ndarray], width: int, pad_id: int, device):
    """ids [B, width] right-padded and their next-token targets (-1 at the last token of a row and at pads)."""
    ids = np.full((len(rows), width), pad_id, dtype=np.int64)
    tgt = np.full((len(rows), width), -1, dtype=np.int64)
    for b, r in enumerate(rows):
        ids[b, :r.size] = r
        tgt[b, :r.size - 1] = r[1:]
    return torch.from_numpy(ids).to(device), torch.from_numpy(tgt).to(device)


def score_variants(reference: str, variants: Sequence[str], model, tokenizer: CharLevelTokenizer, reduce_method: str = "mean",
                   checkpoint_every: int = 512, max_batch_tokens: int = 65536, max_rows_per_pass: int = 64,
                   device: str = "cuda:0") -> VariantScores:
    """Zero-shot variant-effect scores of full-sequence `variants` (substitutions, multi-mutants, insertions, deletions, truncations)
    of one `reference`: `score` as score_sequences would give it, and `delta` = log-likelihood(variant) - log-likelihood(reference),
    summed over all tokens -- the effect of a change on its whole suffix.

    On the engine (one GPU) the reference is forwarded ONCE through the cache path, in chunks that end at the checkpoints in use
    (multiples of `checkpoint_every`, itself a multiple of 64), keeping its per-token log-probs, its attention K / V and a snapshot of
    the Hyena cache per checkpoint.  Variants whose first change lies behind a checkpoint c (plan_variants) are forwarded from c only:
    the Hyena layers start from the snapshot, rotary from position c, and attention reads the reference's K / V [:c] in place
    (HipOps.attention_prefix: no per-row copy of the prefix).  Row 0 of every pass is the reference's own suffix, so that
    delta = sum_{t >= c} lp_v[t] - sum_{t >= c} lp_row0[t] is a PAIRED difference (same launches, same carry-in).  Any other model
    object takes one full forward per batch of variants (reference in row 0).  A variant equal to the reference costs nothing:
    delta 0.0, first_diff -1."""
    if reduce_method not in ("mean", "sum"):
        raise ValueError(f"Invalid reduce_method {reduce_method}")
    ref = _bos_ids(reference, tokenizer)
    vids = [_bos_ids(v, tokenizer) for v in variants]
    if ref.size < 2 or any(v.size < 2 for v in vids):
        raise ValueError("score_variants: empty sequence")
    engine = hasattr(model, "hidden_states") and hasattr(getattr(model, "ops", None), "attention_prefix")
    plan = plan_variants(ref, vids, checkpoint_every, max_batch_tokens, max_rows_per_pass, cached=engine)
    red = (lambda tot, n: tot / n) if reduce_method == "mean" else (lambda tot, n: tot)
    N, Tr = len(vids), ref.size
    pad = tokenizer.pad_id
    lp_ref, snaps, shared = None, {}, None
    if engine and plan.checkpoints:
        from .sh.cache import InferenceParams, RecurrentInferenceParams, SharedPrefix
        cache = model.initialize_inference_params()
        cache["mha"].max_seqlen = Tr
        ids_r, tgt_r = _padded([ref], Tr, pad, device)
        edges = [0] + list(plan.checkpoints) + [Tr]
        parts = []
        for a, b in zip(edges[:-1], edges[1:]):
            # (a chunk may be ONE token long -- the reference ends right behind a checkpoint that a longer variant uses: the
            #  cache path then runs it as a decode step)
            if a > 0:                                                  # the Hyena cache entering checkpoint a (about 7 MB at 7B)
                hy = cache["hyena"]
                snaps[a] = ({i: t.clone() for i, t in hy.fir_state_dict.items()}, {i: t.clone() for i, t in hy.state_dict.items()})
            cache["mha"].seqlen_offset = cache["hyena"].seqlen_offset = a
            parts.append(_logprobs_of(model, ids_r[:, a:b], tgt_r[:, a:b], cache)[0])
        lp_ref = np.concatenate(parts)[:Tr - 1]
        kvs = dict(cache["mha"].key_value_memory_dict)
        vt = {}
        if model.ops.supports("attention_prefix_vt"):                  # one V^T plane per attention layer, every checkpoint reads its first columns
            vt = {i: model.ops.attention_prefix_vt(kv[0, :plan.checkpoints[-1], 1]) for i, kv in kvs.items()}
        shared = SharedPrefix(kv=kvs, vt=vt)
    delta = np.zeros(N, dtype=np.float64)
    tail = np.zeros(N, dtype=np.float64)                              # sum_{t >= c} lp_v[t]
    row0_full = None
    for g in plan.groups:
        c = g.checkpoint
        rows = [ref[c:]] + [vids[n][c:] for n in g.index]
        ids_g, tgt_g = _padded(rows, g.width, pad, device)
        ipd = None
        if c > 0:
            fir, st = snaps[c]
            ipd = {"mha": InferenceParams(max_seqlen=c + g.width, max_batch_size=g.rows, seqlen_offset=c, shared_prefix=shared),
                   "hyena": RecurrentInferenceParams(fir_filter_length=model.short_filter_length, state_dim=model.state_size, seqlen_offset=c,
                                                     fir_state_dict={i: t.expand(g.rows, *t.shape[1:]).contiguous() for i, t in fir.items()},
                                                     state_dict={i: t.expand(g.rows, *t.shape[1:]).contiguous() for i, t in st.items()})}
        lp = _logprobs_of(model, ids_g, tgt_g, ipd)
        s0 = lp[0, :Tr - c - 1].sum()
        if c == 0 and lp_ref is None and row0_full is None:
            row0_full = lp[0, :Tr - 1].copy()
        for b, n in enumerate(g.index, start=1):
            tail[n] = lp[b, :vids[n].size - c - 1].sum()
            delta[n] = tail[n] - s0
    if lp_ref is None:                                                # (no checkpoint in use: the reference's log-probs come from a row 0)
        if row0_full is None:
            ids_r, tgt_r = _padded([ref], Tr, pad, device)
            row0_full = _logprobs_of(model, ids_r, tgt_r, None)[0, :Tr - 1]
        lp_ref = row0_full
    ref_sum = float(lp_ref.sum())
    head = np.concatenate([[0.0], np.cumsum(lp_ref)])                 # head[c] = sum_{t < c} lp_ref[t]
    score = np.empty(N, dtype=np.float64)
    for n in range(N):
        if plan.first_diff[n] < 0:
            score[n] = red(ref_sum, Tr - 1)
        else:
            score[n] = red(head[plan.checkpoint[n]] + tail[n], vids[n].size - 1)
    stats = {"tokens": plan.tokens, "naive_tokens": plan.naive_tokens, "passes": len(plan.groups), "checkpoints": list(plan.checkpoints),
             "cached": bool(engine)}
    return VariantScores(score, delta, plan.first_diff, red(ref_sum, Tr - 1), stats)
