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
    return (ops is not None and getattr(ops, "name", "") == "hip-gfx950" and hasattr(ops, "unembed_logprob")
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
    if _fused_tail_ok(model, input_ids) and hasattr(model.ops, "unembed_profile"):
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
    it is conditioned on the prefix only.  What a substitution does to the likelihood of the SUFFIX needs a forward per
    variant and is not computed here."""
    return profile.token_logprobs - profile.logprob[:, None]


def predicted_tokens(profile: PositionProfile) -> np.ndarray:
    """[L] int64: at every position the id, among `profile.tokens`, the model gives the highest probability."""
    return np.asarray(profile.tokens, dtype=np.int64)[profile.token_logprobs.argmax(-1)]


def renormalized(profile: PositionProfile) -> np.ndarray:
    """[L, n]: log-probs renormalised over `profile.tokens` alone (a log-softmax over the columns, in fp64 -> f32)."""
    x = profile.token_logprobs.astype(np.float64)
    m = x.max(-1, keepdims=True)
    return (x - m - np.log(np.exp(x - m).sum(-1, keepdims=True))).astype(np.float32)
