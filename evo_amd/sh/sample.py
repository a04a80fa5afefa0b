"""`stripedhyena.sample` mirror [REF evo/generation.py:7,162-167]."""
import torch


def modify_logits_for_top_k_filtering(logits: torch.Tensor, top_k: int) -> None:
    """Keep the top_k largest logits of each row, set the rest to -inf (in place)."""
    kth = torch.topk(logits, top_k, dim=-1)[0][..., -1, None]
    logits.masked_fill_(logits < kth, float("-inf"))


def modify_logits_for_top_p_filtering(logits: torch.Tensor, top_p: float) -> None:
    """Drop the low-probability tail whose cumulative mass is <= 1 - top_p (in place)."""
    if top_p <= 0.0 or top_p >= 1.0:
        return
    sorted_logits, sorted_idx = torch.sort(logits, descending=False)
    cum = sorted_logits.softmax(dim=-1).cumsum(dim=-1)
    drop_sorted = cum <= (1.0 - top_p)
    drop = drop_sorted.scatter(1, sorted_idx, drop_sorted)
    logits.masked_fill_(drop, float("-inf"))


def sample(logits: torch.Tensor, top_k: int = 1, top_p: float = 0.0, temperature: float = 1.0) -> torch.Tensor:
    """[B, V] logits -> [B] int64 token ids.  top_k == 1 is greedy; otherwise top-k filter, divide by
    temperature, top-p filter, then one multinomial draw."""
    logits = logits.float()
    if top_k == 1:
        return logits.argmax(dim=-1)
    logits = logits.clone()
    if top_p > 0.0:
        assert top_p <= 1.0, "top-p should be in (0, 1]."
    if top_k > 0:
        modify_logits_for_top_k_filtering(logits, min(top_k, logits.size(-1)))
    if temperature != 1.0 and temperature > 0.0:
        logits /= temperature
    modify_logits_for_top_p_filtering(logits, top_p)
    return torch.multinomial(torch.softmax(logits, dim=-1), num_samples=1).squeeze(dim=-1)


# ---------------------------------------------------------------------------------------------------------------------
# Seeded sampling: the written specification of `evo_sample_rows_f32` (csrc/sample.hip).  Pure
# torch / numpy on the CPU, fp64 inside.  A sample's n-th random number is a function of (seed, stream, n) alone.

_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_M32 = 0xFFFFFFFF
VOCAB_BITS = 512


def philox4x32_10(counter, key):
    """Philox4x32 with 10 rounds (Salmon et al., SC'11): counter = 4 and key = 2 words of 32 bits -> 4 words.
    The words are Python ints or numpy uint64 arrays holding 32-bit values (arrays give arrays, element by element)."""
    import numpy as np
    vec = any(isinstance(w, np.ndarray) for w in tuple(counter) + tuple(key))
    cast = (lambda w: np.asarray(w, dtype=np.uint64)) if vec else int
    c0, c1, c2, c3 = (cast(w) & cast(_M32) for w in counter)
    k0, k1 = (cast(w) & cast(_M32) for w in key)
    m32, s32 = cast(_M32), cast(32)
    for _ in range(10):
        p0, p1 = cast(_PHILOX_M0) * c0, cast(_PHILOX_M1) * c2          # 32 x 32 -> 64 bits: fits a uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ k0, p1 & m32, (p0 >> s32) ^ c3 ^ k1, p0 & m32
        k0, k1 = (k0 + cast(_PHILOX_W0)) & m32, (k1 + cast(_PHILOX_W1)) & m32
    return c0, c1, c2, c3


def seeded_uniform(seed, stream, count):
    """u in (0, 1) of draw number `count` of sample `stream` under `seed`: key = (seed low, seed high), counter =
    (stream low, stream high, count low, count high) as 64-bit two's complement, u = ((x0 >> 8) + 0.5) * 2^-24.
    `stream` / `count` may be ints (-> float) or integer arrays (-> float64 array)."""
    import numpy as np
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    if isinstance(stream, (int, np.integer)) and isinstance(count, (int, np.integer)):
        st, ct = int(stream) & 0xFFFFFFFFFFFFFFFF, int(count) & 0xFFFFFFFFFFFFFFFF
        x0 = philox4x32_10((st & _M32, st >> 32, ct & _M32, ct >> 32), (seed & _M32, seed >> 32))[0]
        return ((x0 >> 8) + 0.5) * 2.0 ** -24
    st, ct = np.broadcast_arrays(np.asarray(stream, dtype=np.int64).astype(np.uint64),
                                 np.asarray(count, dtype=np.int64).astype(np.uint64))
    m32, s32 = np.uint64(_M32), np.uint64(32)
    x0 = philox4x32_10((st & m32, st >> s32, ct & m32, ct >> s32),
                       (np.full(st.shape, seed & _M32, dtype=np.uint64), np.full(st.shape, seed >> 32, dtype=np.uint64)))[0]
    return ((x0 >> np.uint64(8)).astype(np.float64) + 0.5) * 2.0 ** -24


def allowed_mask(tokenizer, allowed) -> torch.Tensor:
    """The 512-bit allow mask as a bool tensor [512]: `allowed` is a string (its characters, through `tokenizer`) or
    an iterable of token ids.  An empty set, or an id outside [0, 512), is a ValueError."""
    if isinstance(allowed, torch.Tensor):
        allowed = allowed.tolist()
    ids = [int(t) for t in tokenizer.tokenize(allowed)] if isinstance(allowed, str) else [int(t) for t in allowed]
    if not ids:
        raise ValueError("allowed_tokens: the set of allowed tokens is empty")
    mask = torch.zeros(VOCAB_BITS, dtype=torch.bool)
    for t in ids:
        if not 0 <= t < VOCAB_BITS:
            raise ValueError(f"allowed_tokens: token id {t} is outside [0, {VOCAB_BITS})")
        mask[t] = True
    return mask


def seeded_distribution(logits: torch.Tensor, top_k: int, top_p: float, temperature: float, allowed=None):
    """What a seeded draw is taken from.  logits [B, V] -> (order [B, V] int64, cdf [B, V] fp64, n_kept [B]):
    `order` lists each row's tokens by descending (masked) logit, ties by ascending token id; the kept tokens are its
    first `n_kept`; `cdf` is the inclusive cumulative softmax of the kept tokens in that order (1 beyond them).

    The kept set is the one the filters above keep -- they are called here, on the fp64 rows.  One thing they leave
    open is pinned: when the top-p cut falls inside a group of EQUAL logits, which members go depends on the tie
    order of a non-stable `torch.sort`; here (and in the kernel) the group loses its highest token ids first, i.e. the
    cut is taken in the exact reverse of `order`.  The number of tokens kept of every value is the filters' own."""
    raw = logits.detach().to("cpu", torch.float64)
    if raw.dim() != 2:
        raise ValueError("logits must be [B, V]")
    if allowed is not None:
        raw = raw.masked_fill(~torch.as_tensor(allowed, dtype=torch.bool)[None, :], float("-inf"))
    order = torch.sort(raw, dim=-1, descending=True, stable=True)[1]
    col = torch.arange(raw.shape[1])[None, :]
    if top_k == 1:                                                    # greedy: no filter, no temperature
        n_kept = torch.ones(raw.shape[0], dtype=torch.long)
        xs = raw
    else:
        x = raw.clone()
        if top_p > 0.0:
            assert top_p <= 1.0, "top-p should be in (0, 1]."
        if top_k > 0:
            modify_logits_for_top_k_filtering(x, min(top_k, x.size(-1)))
        if temperature != 1.0 and temperature > 0.0:
            x /= temperature
        modify_logits_for_top_p_filtering(x, top_p)
        n_kept = (x > float("-inf")).sum(-1)
        xs = raw / temperature if (temperature != 1.0 and temperature > 0.0) else raw
    xs = xs.gather(-1, order).masked_fill(col >= n_kept[:, None], float("-inf"))
    cdf = xs.softmax(-1).cumsum(-1)
    cdf = torch.where(col >= (n_kept[:, None] - 1), torch.ones_like(cdf), cdf)
    return order, cdf, n_kept


def sample_seeded(logits: torch.Tensor, top_k: int, top_p: float, temperature: float, seed: int, stream, count,
                  allowed=None) -> torch.Tensor:
    """[B, V] (or [V]) logits -> [B] (or scalar) int64 token ids: the filters of `sample`, then ONE draw per row by
    inverting the CDF of the kept tokens taken in descending-logit order, ties by ascending token id -- the first
    position whose inclusive CDF exceeds u = seeded_uniform(seed, stream[b], count[b]).  top_k == 1 is the arg-max
    (lowest id on ties).  `stream` / `count`: an int for every row or one per row.  `allowed`: bool mask [V] or None."""
    import numpy as np
    single = logits.dim() == 1
    lg = logits[None] if single else logits
    order, cdf, n_kept = seeded_distribution(lg, top_k, top_p, temperature, allowed)
    B = lg.shape[0]
    st = np.broadcast_to(np.asarray(stream, dtype=np.int64), (B,))
    ct = np.broadcast_to(np.asarray(count, dtype=np.int64), (B,))
    u = torch.from_numpy(np.ascontiguousarray(seeded_uniform(seed, st, ct)))
    pos = (cdf <= u[:, None]).sum(-1).clamp_(max=lg.shape[1] - 1)
    pos = torch.minimum(pos, n_kept - 1) if top_k != 1 else torch.zeros_like(pos)
    tok = order.gather(-1, pos[:, None])[:, 0]
    return tok[0] if single else tok


# ---------------------------------------------------------------------------------------------------------------------
# Job control: the written specification of the epilogue of `evo_sample_rows_ctl_f32` (csrc/sample.hip).
# A row with `cnt` tokens recorded draws its token exactly as `sample_seeded` does, records it at position cnt (n = cnt + 1 tokens
# then), and ends for the FIRST reason that holds: the token is a stop token; n is a multiple of `stop_frame` and the last tokens
# (the new one included) spell a stop pattern no longer than n; n >= limit.  The token that ends a job is part of it.

FINISH_RUNNING, FINISH_STOP_TOKEN, FINISH_STOP_SEQUENCE, FINISH_LENGTH = 0, 1, 2, 3
FINISH_NAMES = {FINISH_STOP_TOKEN: "stop_token", FINISH_STOP_SEQUENCE: "stop_sequence", FINISH_LENGTH: "length"}
MAX_STOP_SEQUENCES = 8
MAX_STOP_SEQUENCE_LEN = 8


def stop_patterns(tokenizer, stop_sequences):
    """Strings (through `tokenizer`) or id lists -> a list of id lists.  At most 8 patterns of 1 to 8 tokens each; anything else is a
    ValueError."""
    if stop_sequences is None:
        return []
    if isinstance(stop_sequences, str):
        stop_sequences = [stop_sequences]
    pats = []
    for p in stop_sequences:
        if isinstance(p, torch.Tensor):
            p = p.tolist()
        ids = [int(t) for t in tokenizer.tokenize(p)] if isinstance(p, str) else [int(t) for t in p]
        if not 1 <= len(ids) <= MAX_STOP_SEQUENCE_LEN:
            raise ValueError(f"stop_sequences: a pattern has 1 to {MAX_STOP_SEQUENCE_LEN} tokens, got {len(ids)}")
        if any(not 0 <= t < VOCAB_BITS for t in ids):
            raise ValueError(f"stop_sequences: a token id of {ids} is outside [0, {VOCAB_BITS})")
        pats.append(ids)
    if len(pats) > MAX_STOP_SEQUENCES:
        raise ValueError(f"stop_sequences: at most {MAX_STOP_SEQUENCES} patterns, got {len(pats)}")
    return pats


def pack_stop_sequences(patterns):
    """Id lists (see `stop_patterns`) -> (int32 [n_seq, 8] padded with -1, int32 [n_seq]) on the host: what the C entry takes."""
    pats = stop_patterns(None, patterns)
    seq = torch.full((len(pats), MAX_STOP_SEQUENCE_LEN), -1, dtype=torch.int32)
    for q, p in enumerate(pats):
        seq[q, : len(p)] = torch.tensor(p, dtype=torch.int32)
    return seq, torch.tensor([len(p) for p in pats], dtype=torch.int32)


def finish_reason(ids, limit: int, stop_tokens=(), stop_sequences=(), stop_frame: int = 1) -> int:
    """`ids`: every token the row has recorded, the new one last (n = len(ids) >= 1).  -> FINISH_* (0: the row goes on).
    `stop_tokens`: a set of ids or a bool mask [512]; `stop_sequences`: id lists."""
    if int(stop_frame) < 1:
        raise ValueError("stop_frame must be >= 1")
    ids = [int(t) for t in ids]
    n, tok = len(ids), ids[-1]
    if isinstance(stop_tokens, torch.Tensor):
        is_stop = bool(stop_tokens[tok])
    else:
        is_stop = stop_tokens is not None and tok in stop_tokens
    if is_stop:
        return FINISH_STOP_TOKEN
    if n % int(stop_frame) == 0:
        for p in stop_sequences or ():
            p = [int(t) for t in p]
            if len(p) <= n and ids[n - len(p):] == p:                # a pattern longer than n reads nothing
                return FINISH_STOP_SEQUENCE
    if n >= int(limit):
        return FINISH_LENGTH
    return FINISH_RUNNING


def stop_point(ids, limit: int, stop_tokens=(), stop_sequences=(), stop_frame: int = 1):
    """Where the rule ends a job whose tokens WOULD be `ids` (at least min(limit, len(ids)) of them): (length, finish).  finish is 0
    when `ids` runs out first."""
    ids = [int(t) for t in ids]
    for n in range(1, len(ids) + 1):
        r = finish_reason(ids[:n], limit, stop_tokens, stop_sequences, stop_frame)
        if r:
            return n, r
    return len(ids), FINISH_RUNNING


def sample_ctl(logits: torch.Tensor, top_k: int, top_p: float, temperature: float, seed: int, stream: int, history, limit: int,
               allowed=None, stop_tokens=(), stop_sequences=(), stop_frame: int = 1, hist_len=None):
    """One launch of the control kernel for one ACTIVE row: logits [V], `history` = the cnt tokens recorded so far ->
    (token or None, tokens recorded now, finish).  A row with cnt >= limit -- or, with a history of `hist_len` cells, cnt >= hist_len --
    ends with FINISH_LENGTH without drawing: token None, the count unchanged."""
    cnt = len(history)
    if cnt >= int(limit) or (hist_len is not None and cnt >= int(hist_len)):
        return None, cnt, FINISH_LENGTH
    tok = int(sample_seeded(logits, top_k, top_p, temperature, seed, stream, cnt, allowed))
    return tok, cnt + 1, finish_reason(list(history) + [tok], limit, stop_tokens, stop_sequences, stop_frame)


# ---------------------------------------------------------------------------------------------------------------------
# Constrained generation: the written specification of `evo_sample_rows_dfa_f32` (csrc/sample.hip).  A row stands in
# state `state` of an automaton `table` [n_states, 8] over the tokens `alphabet` (at most 8): table[q][a] is what drawing alphabet[a] in
# state q does -- >= 0 the next state, DFA_ACCEPT the constraint is complete, any other negative value forbidden.  The state's permitted
# tokens, intersected with the global allow mask, are the allow set of the draw of `sample_ctl`; the drawn token moves the state.

FINISH_CONSTRAINT, FINISH_DEAD_END = 4, 5
FINISH_NAMES_ALL = {**FINISH_NAMES, FINISH_CONSTRAINT: "constraint", FINISH_DEAD_END: "dead_end"}
DFA_ACCEPT = -2
DFA_MAX_SYMBOLS = 8


def dfa_allowed(table, state: int, alphabet, allowed=None) -> torch.Tensor:
    """bool [512]: the tokens state `state` permits (a next state or DFA_ACCEPT on their symbol), and `allowed` (bool [512] or None)
    permits too.  A state outside the table permits nothing."""
    mask = torch.zeros(VOCAB_BITS, dtype=torch.bool)
    if 0 <= int(state) < len(table):
        for a, t in enumerate(alphabet):
            nxt = int(table[int(state)][a])
            if nxt >= 0 or nxt == DFA_ACCEPT:
                mask[int(t)] = True
    if allowed is not None:
        mask &= torch.as_tensor(allowed, dtype=torch.bool)
    return mask


def sample_dfa(logits: torch.Tensor, top_k: int, top_p: float, temperature: float, seed: int, stream: int, history, limit: int, table,
               state, alphabet, allowed=None, stop_tokens=(), stop_sequences=(), stop_frame: int = 1, hist_len=None, base: int = 0):
    """One launch of the automaton kernel for one ACTIVE row -> (token or None, tokens recorded now, finish, new state).  `table` is the
    whole device table, `base` the row of this row's state 0 (base < 0: the row is unconstrained -- `sample_ctl`, the state untouched),
    `state` relative to it.  After `sample_ctl`'s own "nothing left to draw" check: a negative state, base + state outside the table or
    an empty allow set is a dead end -- FINISH_DEAD_END, nothing drawn, count and state unchanged.  Otherwise the draw of `sample_ctl`
    from the state's set; drawing an ACCEPT edge leaves the state and ends the job with FINISH_CONSTRAINT unless a stop token or an
    in-frame stop pattern (which rank first) end it on the same token; the limit ranks last."""
    cnt = len(history)
    if int(base) < 0:
        return sample_ctl(logits, top_k, top_p, temperature, seed, stream, history, limit, allowed, stop_tokens, stop_sequences,
                          stop_frame, hist_len) + (state,)
    if cnt >= int(limit) or (hist_len is not None and cnt >= int(hist_len)):
        return None, cnt, FINISH_LENGTH, state
    r = int(base) + int(state)
    allow = dfa_allowed(table, r if int(state) >= 0 else -1, alphabet, allowed)
    if not bool(allow.any()):
        return None, cnt, FINISH_DEAD_END, state
    tok = int(sample_seeded(logits, top_k, top_p, temperature, seed, stream, cnt, allow))
    nxt = int(table[r][[int(t) for t in alphabet].index(tok)])
    # reasons 1 and 2 first (no limit: it ranks behind the constraint), then acceptance, then the limit
    fin = finish_reason(list(history) + [tok], cnt + 2, stop_tokens, stop_sequences, stop_frame)
    if not fin and nxt == DFA_ACCEPT:
        fin = FINISH_CONSTRAINT
    if not fin and cnt + 1 >= int(limit):
        fin = FINISH_LENGTH
    return tok, cnt + 1, fin, (state if nxt == DFA_ACCEPT else nxt)


# ---------------------------------------------------------------------------------------------------------------------
# Beam search: the written specification of `evo_beam_select_f32` (csrc/beam.hip).  A prompt owns a GROUP of
# W = beam_width consecutive slots g W ... g W + W - 1; G = S // W groups; slots >= G W and groups whose `group_active` is 0 are left
# alone (parent[s] = s, everything else unchanged).  One step, per active group, on the rows the forward produced:
#   * a LIVE beam b (cum[b] > -inf, not ended) offers (b, v) for every allowed token v with score cum[b] + (x[b, v] - lse[b]), in exactly
#     that association; lse[b] is the log-sum-exp of the UNFILTERED row;
#   * an ENDED beam offers itself: score, ids and length unchanged, it stays ended;
#   * an EMPTY beam (cum == -inf) offers nothing;
#   * a candidate whose score is NaN or -inf is none: a NaN logit is never chosen, a row whose lse is NaN or +inf (it holds a NaN or a
#     +inf) offers nothing at all, and a -inf logit would only make an empty beam;
#   * candidates rank by score descending (-0 and +0 are one value), then parent ascending, then token ascending; the best W go to the
#     group's slots in rank order: slot g W + j gets parent (a SLOT index), token, cum, length[parent] + (0 if the parent had ended else 1),
#     ended = parent ended or token in the stop set; with fewer than W candidates the remaining slots become empty: parent = s,
#     cum = -inf, not ended, ids and length unchanged.

def beam_select(logits: torch.Tensor, cum: torch.Tensor, ended: torch.Tensor, length: torch.Tensor, ids: torch.Tensor, beam_width: int,
                group_active=None, allowed=None, stop_tokens=None, dtype=torch.float64):
    """logits [S, V]; cum [S]; ended [S] (bool / u8); length [S]; ids [S] -> (parent, ids, cum, ended, length), new CPU tensors
    (int64, int64, `dtype`, bool, int64); nothing is changed in place.  `allowed` / `stop_tokens`: bool masks [V] or None; `dtype`: what
    the scores are evaluated in (torch.float32 is the kernel's arithmetic, up to the order of the sum inside lse)."""
    W = int(beam_width)
    x = logits.detach().to("cpu").to(dtype)
    if x.dim() != 2:
        raise ValueError("logits must be [S, V]")
    S, V = x.shape
    if not 1 <= W <= 8 or S < W:
        raise ValueError("beam_select: 1 <= beam_width <= 8 and beam_width <= S")
    old_cum = cum.detach().to("cpu").to(dtype).reshape(S)
    old_end = ended.detach().to("cpu").reshape(S).bool()
    old_len = length.detach().to("cpu").reshape(S).to(torch.int64)
    old_ids = ids.detach().to("cpu").reshape(S).to(torch.int64)
    allow = torch.ones(V, dtype=torch.bool) if allowed is None else torch.as_tensor(allowed, dtype=torch.bool).cpu()
    stop = torch.zeros(V, dtype=torch.bool) if stop_tokens is None else torch.as_tensor(stop_tokens, dtype=torch.bool).cpu()
    parent = torch.arange(S, dtype=torch.int64)
    new_ids, new_cum, new_end, new_len = old_ids.clone(), old_cum.clone(), old_end.clone(), old_len.clone()
    lse = torch.logsumexp(x, dim=-1)
    neg_inf = float("-inf")
    for g in range(S // W):
        if group_active is not None and not bool(group_active[g]):
            continue
        cands = []                                                    # (-score, parent, token, score)
        for b in range(g * W, g * W + W):
            c = old_cum[b]
            if not bool(c > neg_inf):                                 # empty (or NaN)
                continue
            if bool(old_end[b]):
                cands.append((-float(c), b, int(old_ids[b]), c))
                continue
            score = c + (x[b] - lse[b])
            ok = allow & (score > neg_inf)                            # (NaN compares false)
            for v in torch.nonzero(ok).reshape(-1).tolist():
                cands.append((-float(score[v]), b, v, score[v]))
        cands.sort(key=lambda t: t[:3])
        for j in range(W):
            s = g * W + j
            if j >= len(cands):
                new_cum[s], new_end[s] = neg_inf, False               # empty; parent = s, ids and length as they were
                continue
            _, b, v, sc = cands[j]
            parent[s], new_ids[s], new_cum[s] = b, v, sc
            new_end[s] = bool(old_end[b]) or bool(stop[v])
            new_len[s] = old_len[b] + (0 if bool(old_end[b]) else 1)
    return parent, new_ids, new_cum, new_end, new_len


# ---------------------------------------------------------------------------------------------------------------------
# k-mer repeat control: the written specification of `evo_repeat_rows_f32` (csrc/repeat.hip).  The launch sits in
# front of the sampler launch of the job-control path.  A job keeps, over an alphabet of n_sym (1 ... 8) distinct token ids and a context
# length k >= 1 (M = n_sym ** k <= 2 ** 20): `counts` int32 [M], how often each k-mer has been seen; the window (code, len): the last
# len <= k - 1 alphabet symbols in base n_sym, newest in the lowest digit; n_gen, the generated tokens folded in, and rep, how many of
# them completed a k-mer that had been seen before.  Per step the token the step is fed is folded in, the rule may end the job
# (FINISH_REPEAT), and otherwise the row the sampler draws from is the model's row minus levels[min(count, 7)] on every symbol, count
# being that of the k-mer the symbol would complete.  Integers and ONE f32 subtraction per symbol: nothing to round differently.

FINISH_REPEAT = 6
FINISH_NAMES_REPEAT = {**FINISH_NAMES_ALL, FINISH_REPEAT: "repeat"}
REPEAT_MAX_SYMBOLS = 8
REPEAT_MAX_TABLE = 1 << 20
REPEAT_LEVELS = 8
REPEAT_END_SCALE = 1024
_COUNT_MAX = 2 ** 31 - 1


class RepeatState:
    """One job's state: counts int32 [M], the window (code, len), (n_gen, rep); `ids` are the alphabet's token ids, `k` the context length."""

    def __init__(self, ids, k: int, counts=None, code: int = 0, length: int = 0, n_gen: int = 0, rep: int = 0):
        self.ids, self.k = tuple(int(t) for t in ids), int(k)
        self.n_sym = len(self.ids)
        self.M = repeat_table_size(self.n_sym, self.k)
        self.counts = torch.zeros(self.M, dtype=torch.int32) if counts is None else torch.as_tensor(counts, dtype=torch.int32).cpu().clone()
        self.code, self.len, self.n_gen, self.rep = int(code), int(length), int(n_gen), int(rep)

    def clone(self):
        return RepeatState(self.ids, self.k, self.counts, self.code, self.len, self.n_gen, self.rep)

    def window(self):
        """(code, len) as the rule reads them: a window outside its invariants (len outside [0, k - 1], code outside [0, n_sym ** (k - 1)))
        reads as the empty one, so that no k-mer index ever leaves [0, M)."""
        if not 0 <= self.len <= self.k - 1 or not 0 <= self.code < self.M // self.n_sym:
            return 0, 0
        return self.code, self.len


def repeat_table_size(n_sym: int, k: int) -> int:
    """M = n_sym ** k; a ValueError outside 1 <= n_sym <= 8, k >= 1, M <= 2 ** 20."""
    n_sym, k = int(n_sym), int(k)
    if not 1 <= n_sym <= REPEAT_MAX_SYMBOLS:
        raise ValueError(f"repeat: the alphabet has 1 to {REPEAT_MAX_SYMBOLS} symbols, got {n_sym}")
    if k < 1:
        raise ValueError(f"repeat: k must be >= 1, got {k}")
    if n_sym == 1:
        return 1
    if k > 20 or n_sym ** k > REPEAT_MAX_TABLE:
        raise ValueError(f"repeat: n_sym ** k = {n_sym} ** {k} exceeds {REPEAT_MAX_TABLE} table cells")
    return n_sym ** k


def repeat_fold(state: RepeatState, token: int, generated: bool) -> RepeatState:
    """Fold one token into `state` (in place; returned for convenience).  A token outside the alphabet empties the window; a symbol at
    len == k - 1 completes the k-mer idx = code * n_sym + a: its count goes up by one (saturating at 2 ** 31 - 1), a GENERATED token that
    completes a k-mer seen before counts as a repeat, and the window moves on; a symbol at len < k - 1 only extends the window.  Every
    generated token, whatever it is, counts in n_gen."""
    code, ln = state.window()
    tok = int(token)
    a = state.ids.index(tok) if tok in state.ids else None
    if a is None:
        code, ln = 0, 0
    elif ln == state.k - 1:
        idx = code * state.n_sym + a
        old = int(state.counts[idx])
        state.counts[idx] = min(old + 1, _COUNT_MAX)
        if generated and old >= 1:
            state.rep += 1
        code = idx % (state.M // state.n_sym)
    else:
        code, ln = code * state.n_sym + a, ln + 1
    if generated:
        state.n_gen += 1
    state.code, state.len = code, ln
    return state


def repeat_init(prompt_ids, control) -> RepeatState:
    """The state a job starts from: every prompt token folded with generated=False (BOS, tag characters and anything else outside the
    alphabet empty the window); with control.count_prompt False the counts are zeroed afterwards -- the window stays, so the first
    generated token completes a k-mer with the prompt's tail.  `control`: anything with `ids`, `k`, `count_prompt` (a resolved
    `RepeatControl`)."""
    state = RepeatState(control.ids, control.k)
    for t in prompt_ids:
        repeat_fold(state, int(t), False)
    if not control.count_prompt:
        state.counts.zero_()
    return state


def repeat_penalise(row: torch.Tensor, state: RepeatState, levels) -> torch.Tensor:
    """row f32 [512] -> a new f32 row.  With len == k - 1, for every symbol a: c = counts[code * n_sym + a] and row[id_a] = row[id_a] -
    levels[min(c, 7)] (a negative c reads as 0) -- one f32 subtraction, nothing else; every other id is untouched.  With len < k - 1 the
    row is unchanged.  `levels`: f32 [8], levels[0] == 0."""
    if row.dtype != torch.float32:
        raise ValueError("repeat_penalise: the row is f32 (a bf16 row is widened first, which is exact)")
    out = row.detach().to("cpu").clone()
    lv = torch.as_tensor(levels, dtype=torch.float32).reshape(REPEAT_LEVELS)
    code, ln = state.window()
    if ln == state.k - 1:
        for a, t in enumerate(state.ids):
            c = int(state.counts[code * state.n_sym + a])
            out[t] = out[t] - lv[min(max(c, 0), REPEAT_LEVELS - 1)]
    return out


def repeat_ended(state: RepeatState, end_num: int, end_min_tokens: int) -> bool:
    """The early end, in integers: armed (end_num > 0), at least end_min_tokens generated tokens folded, and more than end_num / 1024 of
    them repeats."""
    return int(end_num) > 0 and state.n_gen >= int(end_min_tokens) and state.rep * REPEAT_END_SCALE > int(end_num) * state.n_gen


def repeat_row(row: torch.Tensor, state: RepeatState, levels, fed=None, end_num=None, end_min_tokens: int = 1):
    """One ACTIVE row of one launch: fold `fed` (the token the step is fed; None: nothing, a job's first row), then the end rule (`end_num`
    None: not armed), then the penalty -> the f32 row the sampler draws from, or None when the rule ended the job (the caller then clears
    `active`, sets length = count and finish = FINISH_REPEAT)."""
    if fed is not None:
        repeat_fold(state, int(fed), True)
    if end_num is not None and repeat_ended(state, end_num, end_min_tokens):
        return None
    return repeat_penalise(row.detach().to("cpu").float(), state, levels)


class RepeatControl:
    """What `DecodePool.generate(repeat=...)` takes.  `k`: the k-mer length.  `levels`: what is subtracted from a
    symbol's logit when the k-mer it would complete has been seen 0, 1, ... 7 (or more) times -- by default penalty * min(j, max_count),
    otherwise 1 to 8 values, the last one repeated; levels[0] must be 0.  `alphabet`: a string or token ids, 1 to 8 distinct single-byte
    tokens (None: the pool's `allowed_tokens`, else "ACGT").  `count_prompt`: whether the prompt's own k-mers count.  `end_fraction`: a
    job ends (finish "repeat") once more than this fraction of its generated tokens completed a k-mer seen before, after at least
    `end_min_tokens` tokens; None: no early end.  The fraction is held as end_num / 1024."""

    def __init__(self, k: int = 8, penalty: float = 1.0, max_count: int = 4, levels=None, alphabet=None, count_prompt: bool = True,
                 end_fraction=None, end_min_tokens: int = 64):
        self.k, self.penalty, self.max_count, self.levels, self.alphabet = k, penalty, max_count, levels, alphabet
        self.count_prompt, self.end_fraction, self.end_min_tokens = count_prompt, end_fraction, end_min_tokens

    def __repr__(self):
        return (f"RepeatControl(k={self.k!r}, penalty={self.penalty!r}, max_count={self.max_count!r}, levels={self.levels!r}, "
                f"alphabet={self.alphabet!r}, count_prompt={self.count_prompt!r}, end_fraction={self.end_fraction!r}, "
                f"end_min_tokens={self.end_min_tokens!r})")

    def resolve(self, tokenizer=None, allow_mask=None):
        """Everything checked (ValueError) and turned into what the launch takes: `ids` (tuple), `k`, `M`, `levels` (f32 [8], host),
        `end_num` (0: no early end), `end_min_tokens`, `count_prompt`.  `allow_mask`: the pool's bool [512] or None."""
        import math
        from types import SimpleNamespace
        alphabet = self.alphabet
        if alphabet is None:
            alphabet = torch.nonzero(allow_mask).flatten().tolist() if allow_mask is not None else "ACGT"
        if isinstance(alphabet, torch.Tensor):
            alphabet = alphabet.tolist()
        ids = [int(t) for t in tokenizer.tokenize(alphabet)] if isinstance(alphabet, str) and tokenizer is not None \
            else [ord(c) for c in alphabet] if isinstance(alphabet, str) else [int(t) for t in alphabet]
        if not 1 <= len(ids) <= REPEAT_MAX_SYMBOLS or len(set(ids)) != len(ids) or any(not 0 <= t < 256 for t in ids):
            raise ValueError(f"repeat: the alphabet is 1 to {REPEAT_MAX_SYMBOLS} distinct single-byte tokens, got {alphabet!r}")
        if allow_mask is not None and not all(bool(allow_mask[t]) for t in ids):
            raise ValueError("repeat: an alphabet symbol outside allowed_tokens could never be drawn")
        if isinstance(self.k, (bool, float, str)) or int(self.k) != self.k:
            raise ValueError(f"repeat: k must be an integer >= 1, got {self.k!r}")
        M = repeat_table_size(len(ids), int(self.k))
        if self.levels is None:
            if int(self.max_count) < 0:
                raise ValueError("repeat: max_count must be >= 0")
            lv = [float(self.penalty) * min(j, int(self.max_count)) for j in range(REPEAT_LEVELS)]
        else:
            lv = [float(v) for v in self.levels]
            if not 1 <= len(lv) <= REPEAT_LEVELS:
                raise ValueError(f"repeat: levels takes 1 to {REPEAT_LEVELS} values, got {len(lv)}")
            lv = lv + [lv[-1]] * (REPEAT_LEVELS - len(lv))
        levels = torch.tensor(lv, dtype=torch.float64).to(torch.float32)
        if not bool(torch.isfinite(levels).all()):
            raise ValueError(f"repeat: levels must be finite in f32, got {lv}")
        if float(levels[0]) != 0.0:
            raise ValueError(f"repeat: levels[0] (a k-mer never seen) must be 0, got {lv[0]}")
        end_num = 0
        if self.end_fraction is not None:
            f = float(self.end_fraction)
            if not (math.isfinite(f) and 0.0 < f < 1.0):
                raise ValueError(f"repeat: end_fraction must lie in (0, 1), got {self.end_fraction!r}")
            end_num = int(round(f * REPEAT_END_SCALE))
            if not 1 <= end_num <= REPEAT_END_SCALE - 1:
                raise ValueError(f"repeat: end_fraction {f} is held as a multiple of 1 / {REPEAT_END_SCALE} in 1 ... {REPEAT_END_SCALE - 1}")
        if int(self.end_min_tokens) < 1:
            raise ValueError("repeat: end_min_tokens must be >= 1")
        return SimpleNamespace(ids=tuple(ids), n_sym=len(ids), k=int(self.k), M=M, levels=levels, end_num=end_num,
                               end_min_tokens=int(self.end_min_tokens), count_prompt=bool(self.count_prompt))
