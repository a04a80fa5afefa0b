"""TEST INFRASTRUCTURE (never imported by the product): EXACT inputs and the judge for the attention kernels (csrc/attn.hip,
csrc/attn_w64.hip), as tests/dense_exact.py is for the dense layers.  Everything here is eager torch on whatever device is asked for; no
kernel of libevo_mi355x.so is called.  tests/test_attn_exact_host.py pins the designs on the CPU, tests/test_gpu_attn_exact.py uses them.

The idea: an attention row is decided by WHICH KEYS it sees.  The inputs below make every softmax weight exactly 1 or exactly 0, so a
row's output is a closed form of its key multiset and one wrong key -- one too many behind the diagonal, one lost at a tile, split or
segment seam, one counted twice -- changes bf16 patterns instead of hiding in rounding noise.

Scores.  Head dim 128, bf16.  q and k are nonzero in two or three dims (`dims`, varied between cases so every K fragment is used); a
score is a sum of at most three products of bf16 integers, every partial sum a multiple of G = 2,048 below 2^24 G: exact in fp32 in any
order.  One data set serves both forms: plain (softmax_scale = 2^-3.5, the kernels' constant c = softmax_scale log2(e) = 0.12753: an
exponent is c times the score) and PRE (`prescaled`: the score IS the exponent).  Two distinct levels differ by at least G in score,
i.e. 261 log2 units after c (2,048 in PRE) -- 2^-150 is 0 in fp32, and in PRE every nonzero level lies beyond W_THRP = 64.
  U   q = 0, k arbitrary finite data: every visible key has weight 1; the output is the mean of V over the visible keys
  D   exponent G j:  k[j] = (j div 64, j mod 64) [three dims past 16,384 keys: (j div 4096, (j div 64) mod 64, j mod 64)], q = (64 G, G)
      [(4096 G, 64 G, G)]: the output is V[the row's last visible key]
  D'  exponent -G j (q negated): every row returns V[0]
  S   exponent 0 except planted keys t_1 < t_2 < ... with heights G, 2 G, ...: V[t_m] for the last planted key at or before the row's
      limit, the U mean in front of t_1
Values.
  V_id    distinct finite normal bf16 patterns: all 7 mantissa bits, both signs, exponents 2^-30 .. 2^30; a hash of (b, h, key, dim)
  V_hist  V[j, d] = s_bh if d == j mod 128 else 0, s_bh a power of two per (b, h): the sums are key COUNTS per residue class (<= 65 up
          to 8,229 keys), exact in fp32; one key dropped or doubled moves an output by >= 1.9 bf16 spacings at 8,229 keys (7.4 at 2,049, 123 at 64)
  V_alt   the same with sign (-1)^(j div 128): prefix sums stay in {0, 1}, a dropped key flips an output between 0 and 1 / n at ANY
          length.  It cannot see a lost run of 256 ALIGNED keys (128 of each sign per class cancel); V_hist at the shorter lengths does.
Keys inside Tk that no query may see hold finite canaries (2^100): a masked weight is an exact 0 and 0 * 2^100 = 0, while 0 * NaN
would be NaN by IEEE.  Everything behind the tensors / a row's position is 0xFF (NaN): the callers' business (tests/arena.py).

The reference is general: `expected(levels, v, mult)` takes the exponent LEVEL of every key and a multiplicity matrix (how often query
i counts key j) and returns the fp64 mean of V over the visible keys of the highest level -- for the true causal multiplicities these
are the closed forms above; with an edited matrix it says what a kernel with that defect would return (the host tests' wrong key sets).

A fifth design, G (graded weights: every weight an exact power of two, so the WEIGHTING of keys is judged to the bit as well), with its
own reference `expected_graded`, judge `judge_graded` and case lists stands at the end of this file; tests/test_attn_graded_host.py
pins it on the CPU, tests/test_gpu_attn_graded.py uses it.
"""
import math

import torch

HD = 128
G = 2048                                   # score step between two levels
SCALE = 1.0 / math.sqrt(HD)                # softmax_scale = 2^-3.5
C_LOG2 = SCALE * 1.4426950408889634        # the kernels' c = 0.12753: G c = 261 log2 units
W_THR, W_THRP = 32.0, 64.0                 # csrc/attn_w64.hip: deferred-max thresholds (plain / PRE)
CANARY = 2.0 ** 100
DIMS2 = ((0, 1), (63, 64), (126, 127))
DIMS3 = ((0, 64, 127), (7, 8, 120))
HIST_MAX_KEYS = 8229                       # V_hist: counts <= 65, >= 1.9 bf16 spacings per key
ALLOW_REL = 2.0 ** -21                     # U rows: the adjacent pattern only this close (relative) to the rounding boundary
ALLOW_SHARE = 1e-3                         # ... and for at most 0.1 % of a case's elements
BF = torch.bfloat16


def _s64(v):
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= (1 << 63) else v


_C1, _C2, _C3 = _s64(0x9E3779B97F4A7C15), _s64(0xBF58476D1CE4E5B9), _s64(0x94D049BB133111EB)


def mix31(idx, seed):
    """int64 tensor -> int64 in [0, 2^31): a splitmix64-style mix in wrapping int64 arithmetic, the same on every device."""
    z = idx * _C1 + _s64((int(seed) + 1) * _C3)
    z = (z ^ ((z >> 30) & ((1 << 34) - 1))) * _C2
    z = (z ^ ((z >> 27) & ((1 << 37) - 1))) * _C3
    z = z ^ ((z >> 31) & ((1 << 33) - 1))
    return (z >> 33) & 0x7fffffff


def _index(B, T, H, device):
    """[B, T, H, 128] int64: a distinct number per (b, key, h, dim) that does not depend on B, T or H."""
    b = torch.arange(B, dtype=torch.int64, device=device)[:, None, None, None]
    t = torch.arange(T, dtype=torch.int64, device=device)[None, :, None, None]
    h = torch.arange(H, dtype=torch.int64, device=device)[None, None, :, None]
    d = torch.arange(HD, dtype=torch.int64, device=device)[None, None, None, :]
    return ((b * 64 + h) * (1 << 20) + t) * HD + d


# ------------------------------------------------------------------------------------------------ values
def v_id(B, T, H, seed=0, device="cpu"):
    """[B, T, H, 128] bf16: sign | exponent 97 .. 157 (2^-30 .. 2^30) | 7 mantissa bits from a hash of (b, h, key, dim)."""
    z = mix31(_index(B, T, H, device), 11 + seed)
    pat = ((z & 1) << 15) | ((97 + (z >> 8) % 61) << 7) | ((z >> 1) & 127)
    pat = torch.where(pat >= 32768, pat - 65536, pat)
    return pat.to(torch.int16).view(BF)


def head_factor(B, H, device="cpu"):
    """s_bh [B, 1, H, 1] fp64: a power of two per (batch row, head), 2^-3 .. 2^3."""
    bh = torch.arange(B * H, dtype=torch.int64, device=device).reshape(B, 1, H, 1)
    return torch.ldexp(torch.ones((), dtype=torch.float64, device=device), ((bh * 5 + 2) % 7 - 3).to(torch.int32))


def v_hist(B, T, H, device="cpu", alt=False, key0=0):
    """V_hist (alt: V_alt).  key0: the number of the first key (a suffix that continues a prefix's count)."""
    j = torch.arange(key0, key0 + T, dtype=torch.int64, device=device)
    d = torch.arange(HD, dtype=torch.int64, device=device)
    one = ((j % HD)[:, None] == d[None, :]).double()
    if alt:
        one = one * (1.0 - 2.0 * ((j // HD) % 2).double())[:, None]
    return (one[None, :, None, :] * head_factor(B, H, device)).to(BF)


def ordinal(x):
    """bf16 -> int64 such that adjacent bf16 values have adjacent numbers (sign-magnitude patterns unfolded)."""
    p = x.contiguous().view(torch.int16).to(torch.int64) & 0xffff
    mag = p & 0x7fff
    return torch.where(p >= 32768, -mag, mag)


def min_distinct_dims(v, span=64):
    """min over (b, h, j, 1 <= dj <= span) of the number of dims in which V[j] and V[j + dj] differ by MORE than one bf16 ulp."""
    o = ordinal(v)
    worst = HD
    for dj in range(1, min(span, v.shape[1] - 1) + 1):
        worst = min(worst, int(((o[:, dj:] - o[:, :-dj]).abs() > 1).sum(-1).min()))
    return worst


# ------------------------------------------------------------------------------------------------ scores
def key_digits(j, n_dims):
    if n_dims == 2:
        return [j // 64, j % 64]
    return [j // 4096, (j // 64) % 64, j % 64]


def q_weights(n_dims):
    return [64 * G, G] if n_dims == 2 else [4096 * G, 64 * G, G]


def make_qk(design, B, Tq, Tk, H, dims, planted=None, device="cpu"):
    """-> q [B, Tq, H, 128], k [B, Tk, H, 128] bf16 and the exponent LEVELS [B, Tk] int64 (the score of key j in units of G; every
    query of a design carries the same q).  planted: for S, one ascending list of key numbers per batch row."""
    q = torch.zeros(B, Tq, H, HD, dtype=torch.float64, device=device)
    k = torch.zeros(B, Tk, H, HD, dtype=torch.float64, device=device)
    j = torch.arange(Tk, dtype=torch.int64, device=device)
    if design == "U":
        for n, d in enumerate(dims):                                   # arbitrary finite data: integers in [-8, 8] per (b, key, h)
            z = mix31(_index(B, Tk, H, device)[..., d], 70 + n)
            k[..., d] = (z % 17 - 8).double()
        lev = torch.zeros(B, Tk, dtype=torch.int64, device=device)
    elif design in ("D", "D'"):
        assert Tk <= (16384 if len(dims) == 2 else 64 * 4096)
        sign = 1.0 if design == "D" else -1.0
        for d, dig, w in zip(dims, key_digits(j, len(dims)), q_weights(len(dims))):
            k[..., d] = dig.double()[None, :, None]
            q[..., d] = sign * w
        lev = (j if design == "D" else -j)[None, :].expand(B, Tk).contiguous()
    elif design == "S":
        lev = torch.zeros(B, Tk, dtype=torch.int64, device=device)
        z = mix31(_index(B, Tk, H, device)[..., dims[1]], 90)
        k[..., dims[1]] = (z % 17 - 8).double()                        # the second dim: data on k, 0 on q
        q[..., dims[0]] = float(G)
        for b in range(B):
            ts = [t for t in planted[b] if 0 <= t < Tk]
            assert ts == sorted(set(ts)) and len(ts) < 128
            if ts:
                idx = torch.tensor(ts, dtype=torch.int64, device=device)
                lev[b, idx] = torch.arange(1, len(ts) + 1, dtype=torch.int64, device=device)
        k[..., dims[0]] = lev.double()[:, :, None]
    else:
        raise ValueError(design)
    return q.to(BF), k.to(BF), lev


def plant_values(v, v_rows, planted):
    """S: the planted keys of batch row b take their rows from v_rows (V_id), the rest of v (V_hist) stays."""
    for b, ts in enumerate(planted):
        ts = [t for t in ts if 0 <= t < v.shape[1]]
        if ts:
            idx = torch.tensor(ts, dtype=torch.int64, device=v.device)
            v[b, idx] = v_rows[b, idx]
    return v


def put_canaries(k, v, first_unseen, dims):
    """Keys first_unseen .. Tk - 1 (inside Tk, visible to no query): 2^100 in k's active dims and in all of v."""
    if first_unseen < k.shape[1]:
        for d in dims:
            k[:, first_unseen:, :, d] = CANARY
        v[:, first_unseen:] = CANARY
    return k, v


def scores_int(q, k):
    """The exact scores in int64 [B, H, Tq, Tk] (every entry of these designs is an integer; canaries excluded by the caller)."""
    return torch.einsum("bihd,bjhd->bhij", q.double().to(torch.int64), k.double().to(torch.int64))


# ------------------------------------------------------------------------------------------------ key sets
def causal_mult(B, Tq, Tk, q_pos0, device="cpu", shift=0):
    """[B, Tq, Tk] int64: 1 where query i (position q_pos0 + i) sees key j <= min(q_pos0 + i + shift, Tk - 1).  shift != 0: a wrong limit."""
    i = torch.arange(Tq, dtype=torch.int64, device=device)[:, None]
    j = torch.arange(Tk, dtype=torch.int64, device=device)[None, :]
    return (j <= q_pos0 + i + shift).to(torch.int64)[None].expand(B, Tq, Tk).contiguous()


def decode_mult(positions, Tk, device="cpu", shift=0):
    """[B, 1, Tk] int64: row b's single query at positions[b] sees keys 0 .. positions[b] (+ shift)."""
    p = torch.as_tensor(positions, dtype=torch.int64, device=device)[:, None, None]
    j = torch.arange(Tk, dtype=torch.int64, device=device)[None, None, :]
    return (j <= p + shift).to(torch.int64)


def expected(lev, v, mult):
    """lev [B, Tk] int64, v [B, Tk, H, 128] bf16, mult [B, nq, Tk] int64 -> (ref [B, nq, H, 128] fp64, single [B, nq] bool).
    ref = sum_j w_j V[j] / sum_j w_j with w_j = mult_j where key j is visible AND on the row's highest visible level, else 0 -- the
    softmax of these designs (weights exactly 1 or 0).  single: one key with multiplicity > 0 on that level: ref IS that V row."""
    B, nq, Tk = mult.shape
    H = v.shape[2]
    ref = torch.zeros(B, nq, H, HD, dtype=torch.float64, device=v.device)
    single = torch.zeros(B, nq, dtype=torch.bool, device=v.device)
    low = torch.iinfo(torch.int64).min
    for b in range(B):
        vis = mult[b] > 0
        top = torch.where(vis, lev[b][None, :], torch.full_like(mult[b], low)).max(-1, keepdim=True).values
        w = torch.where(vis & (lev[b][None, :] == top), mult[b], torch.zeros_like(mult[b]))
        cnt = (w > 0).sum(-1)
        single[b] = cnt == 1
        if bool(single[b].all()):
            ref[b] = v[b, w.argmax(-1)].double()
        else:
            n = int(vis.any(0).nonzero().max()) + 1 if bool(vis.any()) else 1
            num = w[:, :n].double() @ v[b, :n].double().reshape(n, H * HD)
            den = w.sum(-1).double().clamp_min(1.0)
            ref[b] = (num / den[:, None]).reshape(nq, H, HD)
    return ref, single


# ------------------------------------------------------------------------------------------------ the judge
def bf16_neighbourhood(v):
    """v fp64 -> (e: v rounded to bf16, as fp64; nb: the bf16 neighbour of e on v's side; dist: |v|'s distance to the rounding
    boundary between the two) -- row 22e's rule (tests/test_gpu_decode_regimes.py)."""
    e = v.float().bfloat16().double()
    a = e.abs()
    m, ex = torch.frexp(a)
    ulp = torch.ldexp(torch.ones_like(a), ex - 8)
    down = torch.where(m > 0.5, ulp / 2, ulp / 4)                       # (below a power of two the spacing halves)
    up_side = v.abs() >= a
    mid = torch.where(up_side, a + ulp / 2, a - down)
    nb = torch.where(up_side, a + ulp, a - 2 * down) * torch.where(e < 0, -1.0, 1.0)
    return e, nb, (v.abs() - mid).abs()


class Verdict:
    """bad [B, nq] bool: rows with an element outside the rule; n_bad: such elements; n_allowed: U elements that took the adjacent
    pattern inside the boundary rule; n_adjacent: exact-row elements one pattern off where the case allows that (see judge)."""

    def __init__(self, bad, n_bad, n_allowed, n_adjacent, n_elems):
        self.bad, self.n_bad, self.n_allowed, self.n_adjacent, self.n_elems = bad, n_bad, n_allowed, n_adjacent, n_elems

    @property
    def ok(self):
        return self.n_bad == 0 and self.n_allowed <= ALLOW_SHARE * self.n_elems

    def __repr__(self):
        return (f"{self.n_bad} mismatching of {self.n_elems} elements in {int(self.bad.sum())} rows, {self.n_allowed} on the boundary allowance "
                f"({100.0 * self.n_allowed / max(1, self.n_elems):.4f} %), {self.n_adjacent} adjacent patterns in rows that may take one")


def judge(got, ref, single, adjacent_rows=None):
    """got [B, nq, H, 128] bf16 against expected()'s (ref, single).  Every element is judged; there is no tensor-wide term.
      single rows   the int16 pattern of got equals that of ref (ref is a bf16 V row).  adjacent_rows [B, nq] bool (default: none): rows
                    that may instead hold the ADJACENT bf16 pattern -- for the plain-form cases whose arithmetic is shown to round the
                    winner's weight (tests/test_gpu_attn_exact.py, `_adjacent_rows`); never a PRE case
      other rows    got == bf16(ref); the adjacent pattern on ref's side only where ref lies within 2^-21 |ref| of the rounding boundary,
                    and (Verdict.ok) for at most 0.1 % of the case's elements."""
    g = got.contiguous()
    e, nb, dist = bf16_neighbourhood(ref)
    gd = g.double()
    s4 = single[:, :, None, None]
    same_bits = g.view(torch.int16) == ref.to(BF).contiguous().view(torch.int16)
    ok_single = same_bits
    adj = torch.zeros_like(same_bits)
    if adjacent_rows is not None:
        adj = (~same_bits) & ((ordinal(g) - ordinal(ref.to(BF))).abs() == 1) & adjacent_rows[:, :, None, None] & s4
        ok_single = same_bits | adj
    eq = gd == e
    allowed = (~eq) & (gd == nb) & (dist <= ALLOW_REL * ref.abs()) & ~s4
    ok = torch.where(s4, ok_single, eq | allowed)
    return Verdict((~ok).any(-1).any(-1), int((~ok).sum()), int(allowed.sum()), int(adj.sum()), got.numel())


# ------------------------------------------------------------------------------------------------ the w64 bookkeeping in plain torch
def emulate_w64(q, k, v, q_pos0, pre, c=None, defect=None):
    """fp32 emulation of attn_fwd_w64_kernel's arithmetic for one (batch row, head): q [Tq, 128], k / v [Tk, 128] bf16 -> [Tq, 128] bf16.
    64-key tiles in order; a row's exponents are taken relative to a reference point: PRE -- 0 while the tile's largest exponent stays
    inside +-W_THRP (a first visible tile may also pull it down), the tile maximum beyond; plain -- the first visible tile's maximum,
    moved when a tile exceeds it by more than W_THR.  P is rounded to bf16 for P.V, l sums the UNROUNDED fp32 weights.
    c: the plain form's scale_log2 (default C_LOG2; design G runs it at 1).  defect: a wrong arithmetic (tests/test_attn_graded_host.py)."""
    Tq, Tk = q.shape[0], k.shape[0]
    qf, kf, vf = q.float(), k.float(), v.float()
    lim = (q_pos0 + torch.arange(Tq)).clamp_max(Tk - 1)
    nm = torch.zeros(Tq)
    seen = torch.zeros(Tq, dtype=torch.bool)
    l = torch.zeros(Tq)
    o = torch.zeros(Tq, HD)
    c = torch.tensor(C_LOG2 if c is None else c, dtype=torch.float32)
    for k0 in range(0, int(lim.max()) + 1, 64):
        kt, vt = kf[k0:k0 + 64], vf[k0:k0 + 64]
        s = (qf.double() @ kt.double().T).float()                                    # exact: see scores_int
        s = s.masked_fill(torch.arange(k0, k0 + kt.shape[0])[None, :] > lim[:, None], float("-inf"))
        e = s + nm[:, None] if pre else (s.double() * c.double() + nm.double()[:, None]).float()       # one rounding: the fma
        emx = e.max(-1).values
        got = emx > float("-inf")
        if pre:
            upd = (emx > W_THRP) | (~seen & got & (emx < -W_THRP))
        else:
            upd = (seen & (emx > W_THR)) | (~seen & got)
        dl = torch.where(upd, emx, torch.zeros_like(emx))
        alpha = torch.where(seen, torch.exp2(-dl), torch.zeros_like(dl))
        nm = nm - dl
        e = e - dl[:, None]
        seen = seen | (got if pre else upd)
        p = torch.exp2(e)
        pb = p.to(BF)
        a_l = a_o = alpha
        if defect is not None:
            if defect in ("skip8", "skip12"):
                p = torch.where(e < e.max(-1, keepdim=True).values - float(defect[4:]), torch.zeros_like(p), p)
                pb = p.to(BF)
            elif defect == "alpha_err":
                a_l = a_o = alpha * (1 + 2.0 ** -10)
            elif defect == "alpha_l_only":
                a_o = torch.where(seen, torch.ones_like(alpha), alpha)
            elif defect == "alpha_o_only":
                a_l = torch.where(seen, torch.ones_like(alpha), alpha)
            elif defect == "trunc_p":
                pb = (p.view(torch.int32) & -65536).view(torch.float32).to(BF)
            else:
                raise ValueError(defect)
        l = l * a_l + p.sum(-1)
        o = o * a_o[:, None] + pb.float() @ vt
    inv = torch.where(l > 0, 1.0 / l, torch.zeros_like(l))
    return (o * inv[:, None]).to(BF)


# ------------------------------------------------------------------------------------------------ split maps (decode)
def stream_split_counts(n_keys, n_splits):
    """attn_decode_stream_kernel: split s takes the 64-key blocks s, s + n_splits, ... -> keys per split."""
    nblk = (n_keys + 63) // 64
    out = [0] * n_splits
    for blk in range(nblk):
        out[blk % n_splits] += min(64, n_keys - 64 * blk)
    return out


def mfma_split_counts(n_keys, n_splits):
    """attn_fwd_kernel<true>: split s takes ceil(n_tiles / n_splits) CONSECUTIVE 64-key tiles -> keys per split."""
    n_tiles = (n_keys + 63) // 64
    per = (n_tiles + n_splits - 1) // n_splits
    out = []
    for s in range(n_splits):
        t0, t1 = s * per, min((s + 1) * per, n_tiles)
        out.append(max(0, min(n_keys, 64 * t1) - 64 * t0) if t0 < t1 else 0)
    return out


# ------------------------------------------------------------------------------------------------ seams
def prefill_seams(Tq, q_pos0, Tk):
    return sorted({t for t in (0, 63, 64, 127, 128, q_pos0 - 1, q_pos0, q_pos0 + 1, Tk - 1, q_pos0 + Tq - 1) if 0 <= t < Tk})


def decode_seams(n_keys, n_splits):
    """Keys 0 / 63 / 64 / 127 / 128, 64 n_splits -+, the first and last key of a ragged 32-key half, the last key of every split's
    first block, the last key."""
    ts = {0, 63, 64, 127, 128, 64 * n_splits - 1, 64 * n_splits, n_keys - 1, (n_keys - 1) // 32 * 32}
    ts |= {64 * s + 63 for s in range(min(n_splits, 24))}
    return sorted(t for t in ts if 0 <= t < n_keys)


# ------------------------------------------------------------------------------------------------ cases (shared by the CPU and the GPU module)
DESIGNS = ("U", "D", "D'", "S")
# (Tq, q_pos0, Tk - (q_pos0 + Tq)): the 64-rows-per-wave kernel; -30: the ragged end decides the last rows; +70: canary keys inside Tk
W64_SHAPES = [(129, 0, 0), (200, 0, 0), (256, 0, 0), (257, 1, 0), (321, 63, 0), (385, 64, 0), (513, 65, 0), (130, 1000, 0),
              (321, 63, -30), (257, 1, 70)]
PIPE_SHAPES = W64_SHAPES[:5]                                            # the 8-wave kernel
QB128_SHAPES = [(128, 0, 0), (128, 63, 0), (128, 64, 0)] + [(Tq, Tk - Tq, 0) for Tk in (200, 2049) for Tq in (1, 37, 64, 128)]
PREFIX_SHAPES = [(P, Tq) for P in (64, 256, 320) for Tq in (129, 257, 321)]
DECODE_POSITIONS = [0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 2080, 8228]
DECODE_SPLITS = [1, 4, 8, 40, 64, 128, None]                            # None: HipOps.attention_decode's default (32); 40: the combine
                                                                        # kernel's 32-split trips AND its tail loop in one (batch, head)
LONG_CAP, LONG_POSITIONS = 131072, [0, 70000, 131071]
MFMA_POSITIONS, MFMA_SPLITS = [0, 63, 64, 2050, 2099], [1, 3, 7, 64]    # attn_fwd_kernel<true>


def prefill_planted(B, Tq, q_pos0, Tk, P=0):
    """S: the planted keys of every batch row.  Every row plants the seams and two keys of its own behind q_pos0 + 1; the LAST row of a
    batch of several (no shared prefix) plants nothing in front of key q_pos0 + 20, so its first 20 rows return the U mean.  P: the
    length of a shared prefix -- its planted keys are the same in every row."""
    base = prefill_seams(Tq, q_pos0, Tk) + ([P - 1, P] if P else [])
    out = []
    for b in range(B):
        ts = set(base) | {t for t in (q_pos0 + 2 + 3 * b, q_pos0 + 66 + b) if t < Tk}
        if b > 0 and b == B - 1 and not P:
            ts = {t for t in ts if t >= q_pos0 + 20}
        out.append(sorted(t for t in ts if 0 <= t < Tk))
    return out


def build_case(design, B, H, nq, q_pos0, Tk, dims, device="cpu", planted=None, shared_prefix=0, alt=False, mult=None):
    """One case: q [B, nq, H, 128], k, v [B, Tk, H, 128] (bf16), levels [B, Tk], the true multiplicities [B, nq, Tk] (causal from
    q_pos0 unless given), the planted keys.  shared_prefix = P: keys 0 .. P - 1 are batch row 0's in every row."""
    if design == "S" and planted is None:
        planted = prefill_planted(B, nq, q_pos0, Tk, shared_prefix)
    q, k, lev = make_qk(design, B, nq, Tk, H, dims, planted, device)
    if design == "U":
        v = v_hist(B, Tk, H, device, alt=alt)
    elif design == "S":
        v = plant_values(v_hist(B, Tk, H, device), v_id(B, Tk, H, 0, device), planted)
    else:
        v = v_id(B, Tk, H, 0, device)
    if shared_prefix:
        P = shared_prefix
        k[:, :P], v[:, :P], lev[:, :P] = k[:1, :P], v[:1, :P], lev[:1, :P]
    if mult is None:
        mult = causal_mult(B, nq, Tk, q_pos0, device)
        k, v = put_canaries(k, v, min(q_pos0 + nq, Tk), dims)
    return {"q": q, "k": k, "v": v, "lev": lev, "mult": mult, "planted": planted, "dims": dims}


def build_decode(design, positions, H, dims, n_splits, device="cpu", alt=False, Tk=None):
    """Decode: batch row b has ONE query at positions[b]; tensors hold max(positions) + 1 keys, what lies behind a row's position is the
    caller's to poison (the multiplicities say which keys count)."""
    B = len(positions)
    Tk = max(positions) + 1 if Tk is None else Tk
    planted = [decode_seams(p + 1, n_splits) for p in positions] if design == "S" else None
    if design == "S":
        planted = [ts[1:] if b % 2 and len(ts) > 1 else ts for b, ts in enumerate(planted)]      # odd rows: the U mean in front of t_1
    return build_case(design, B, H, 1, 0, Tk, dims, device, planted=planted, alt=alt, mult=decode_mult(positions, Tk, device))


# ================================================================================================ design G: graded weights
# The designs above make every softmax weight 1 or 0; they pin WHICH keys a row sees and cannot see how keys are WEIGHTED (every
# rescale factor is 0 or 1).  G makes every weight an exact power of two instead: a score is an integer exponent in log2 units,
#   k[j] = (e_j div 16, e_j mod 16) in two dims, q_i = (16 mu_i, mu_i): score = mu_i e_j, mu_i = G_MUS[i mod 3] (neighbouring rows rank
#   the keys differently), e_j = base_j - g_j with g_j a hash of the key in 0 .. win and base_j piecewise constant (0: FLAT; a list of
#   levels between fixed cuts: STAIR),
# and V = V_hist: output dim d is its own accumulator of s_bh sum 2^(mu e_j) over the keys j = d mod 128.  One data set serves PRE (the
# score IS the exponent) and the plain form at softmax_scale = G_LN2, where the entries' own scale_log2 = softmax_scale * log2(e) is
# 1.0f exactly (tests/test_attn_graded_host.py pins that).
# Exactness (graded_check): ceil(log2(n_keys + 1)) + max|mu| win <= 24.  Then for a flat row every weight 2^n, its bf16 rounding, every
# partial sum of l and of any output dim is exact in fp32 in any order under any common power-of-two reference; only 1 / l and the last
# multiply round (< 1.5 * 2^-24: inside the judge's 2^-21 boundary rule).
# Stair rows mix levels.  Two levels of one list that can meet inside one 64-key tile differ by <= 3 (exact as above: win = 4, <= 640
# keys: 10 + 2 (4 + 3) = 24 bits) or by >= 30 (the lower level's whole tile weighs < 2^-24 of one upper key); across tiles any
# difference costs one fp32 rounding per accumulation.  Hence the allowance of a stair row (graded_allow): (64-key blocks visited +
# non-empty splits + 2) * 2^-24 relative, on the boundary rule, nothing tensor-wide.
# A row's exponents span at most G_SPAN = 100 log2 units (v_exp_f32 flushes below 2^-126; outputs stay normal bf16 numbers), which mu = 2
# allows only for the narrow list N: the wide lists carry mu in (1, -1, 1).
G_MUS = (1, -1, 2)
G_LN2 = 0.6931471824645996                  # an fp32 number; fl32(G_LN2 * 1.4426950408889634f) == 1.0f
G_SPAN = 100
G_SEED = 206                                # of the hash g: one under which no case of the lists has a short row whose common mantissa sits
                                            # on a rounding boundary (a condition on the inputs: test_allowance_zone_share_is_under_the_cap)
G_CUTS = (64, 128, 168, 256, 300, 384, 512, 555)        # tile seams 64 / 128 / 256 (= 64 * 4 splits) / 384 / 512 (= 64 * 8) and mid-tile 168 / 300 / 555
G_MID = (2, 4, 7)                                        # the cuts (by number) that lie inside a tile
# levels between the cuts and the rows' mu.  N: +31 / +32 / +33 around W_THR for mu = +-1 and 62 / 64 / 66 around W_THRP for mu = 2.
# W1: +63 / +64 / +65 around W_THRP, drops of 40 and 70, a rise of 65 from below.  W2: a first visible tile at -65 (PRE pulls its
# reference down), then +32 / +33 / +64 / +65 relative to it; for mu = -1 every list is its mirror image (a first tile at +65, ...).
G_STAIRS = {
    "N": ((0, 31, 32, 33, 1, 33, 0, 32, 33), (1, -1, 2)),
    "W1": ((0, 63, 64, 65, 25, -5, 60, -10, -9), (1, -1, 1)),
    "W2": ((-65, -33, -32, -1, 0, -40, 25, -45, -44), (1, -1, 1)),
}
G_WIN_STAIR = 4                             # stair rows (<= 641 keys)


def graded_win(n_keys):
    """Flat rows: the widest window the exactness condition allows -- 7 up to 1,023 keys (2^-14 for mu = 2: a kernel that skipped weights
    12 or more log2 units down would show), 6 up to 2,049, 5 up to 8,229."""
    return 7 if n_keys <= 1023 else (6 if n_keys <= 2049 else 5)
G_STAIR_MAX_KEYS = 641                      # 11 blocks at most: the prefix case P 320 + Tq 321; the allowance stays <= 2^-20 for prefill


def graded_check(n_keys, win, mus, stair=None, cuts=G_CUTS):
    """The builder's conditions (see above); raises AssertionError."""
    amax = max(abs(m) for m in mus)
    near = 0
    if stair is not None:
        lv = G_STAIRS[stair][0]
        assert n_keys <= G_STAIR_MAX_KEYS and len(lv) == len(cuts) + 1
        assert amax * (max(lv) - min(lv) + win) <= G_SPAN, "a row's exponents leave the span"
        for n in range(len(cuts)):
            d = abs(lv[n + 1] - lv[n])
            if cuts[n] % 64:
                assert d <= 3 or d >= 30, f"levels {lv[n]} | {lv[n + 1]} meet inside a tile"
                near = max(near, d if d <= 3 else 0)
    else:
        assert amax * win <= G_SPAN
    assert math.ceil(math.log2(n_keys + 1)) + amax * (win + near) <= 24, "the integer sums do not fit 24 bits"


def graded_exponents(B, Tk, win, stair=None, cuts=G_CUTS, device="cpu"):
    """e [B, Tk] int64: base - g.  g: a hash of (batch row, key) in 0 .. win, 0 at key 0 and on both sides of every cut (so a level is
    reached where it begins and ends)."""
    j = torch.arange(Tk, dtype=torch.int64, device=device)
    b = torch.arange(B, dtype=torch.int64, device=device)[:, None]
    g = mix31(b * (1 << 20) + j[None, :], G_SEED) % (win + 1)
    base = torch.zeros(Tk, dtype=torch.int64, device=device)
    g[:, 0] = 0
    if stair is not None:
        lv = torch.tensor(G_STAIRS[stair][0], dtype=torch.int64, device=device)
        base = lv[torch.bucketize(j, torch.tensor(cuts, dtype=torch.int64, device=device), right=True)]
        for t in cuts:
            if t < Tk:
                g[:, t - 1:t + 1] = 0
    return base[None, :] - g


def build_graded(B, H, nq, q_pos0, Tk, dims, win, stair=None, device="cpu", mult=None, cuts=G_CUTS, shared_prefix=0, row_mu=False):
    """One G case: q [B, nq, H, 128], k, v [B, Tk, H, 128] bf16, e [B, Tk] int64, mu [B, nq] int64, mult [B, nq, Tk] (causal from q_pos0
    unless given).  row_mu: mu goes by BATCH ROW (decode: one query per row), else by query.  shared_prefix = P: keys 0 .. P - 1 are
    batch row 0's in every row."""
    mus = G_MUS if stair is None else G_STAIRS[stair][1]
    graded_check(Tk, win, mus, stair, cuts)
    e = graded_exponents(B, Tk, win, stair, cuts, device)
    if shared_prefix:
        e[:, :shared_prefix] = e[:1, :shared_prefix]
    sel = torch.arange(B, device=device)[:, None].expand(B, nq) if row_mu else torch.arange(nq, device=device)[None, :].expand(B, nq)
    mu = torch.tensor(mus, dtype=torch.int64, device=device)[sel % 3]
    q = torch.zeros(B, nq, H, HD, dtype=torch.float64, device=device)
    k = torch.zeros(B, Tk, H, HD, dtype=torch.float64, device=device)
    d0, d1 = dims[0], dims[1]
    k[..., d0] = torch.div(e, 16, rounding_mode="floor").double()[:, :, None]
    k[..., d1] = (e % 16).double()[:, :, None]
    q[..., d0] = 16.0 * mu.double()[:, :, None]
    q[..., d1] = mu.double()[:, :, None]
    if mult is None:
        mult = causal_mult(B, nq, Tk, q_pos0, device)
    return {"q": q.to(BF), "k": k.to(BF), "v": v_hist(B, Tk, H, device), "e": e, "mu": mu, "mult": mult, "dims": (d0, d1), "win": win,
            "stair": stair}


def expected_graded(e, mu, v, mult):
    """e [B, Tk] int64, mu [B, nq] int64, v [B, Tk, H, 128] bf16, mult [B, nq, Tk] int64 -> ref [B, nq, H, 128] fp64: the softmax of the
    integer exponents mu_i e_j over the keys with mult > 0, each counted mult times (as in expected(): an edited matrix or an edited mu
    describes a defect).  Weights are exact powers of two (ldexp); the fp64 sums carry 2^-53 relative."""
    B, nq, Tk = mult.shape
    H = v.shape[2]
    ref = torch.zeros(B, nq, H, HD, dtype=torch.float64, device=v.device)
    one = torch.ones((), dtype=torch.float64, device=v.device)
    for b in range(B):
        ex = mu[b][:, None] * e[b][None, :]
        vis = mult[b] > 0
        top = torch.where(vis, ex, torch.full_like(ex, -(1 << 40))).max(-1, keepdim=True).values
        w = torch.where(vis, torch.ldexp(one, (ex - top).clamp_min(-1000).to(torch.int32)), torch.zeros_like(one)) * mult[b].double()
        ref[b] = ((w @ v[b].double().reshape(Tk, H * HD)) / w.sum(-1, keepdim=True).clamp_min(2.0 ** -1000)).reshape(nq, H, HD)
    return ref


def graded_allow(mult, stair, n_splits=0):
    """[B, nq] fp64: the relative half-width of the boundary rule per row.  Flat: ALLOW_REL (two roundings, < 1.5 * 2^-24, sit inside).
    Stair: (64-key blocks visited + non-empty splits + 2) * 2^-24, at most 2^-24 * 22 with <= 640 keys."""
    if stair is None:
        return torch.full(mult.shape[:2], ALLOW_REL, dtype=torch.float64, device=mult.device)
    j = torch.arange(mult.shape[2], device=mult.device)
    last = torch.where(mult > 0, j, torch.zeros_like(j)).max(-1).values
    blocks = last // 64 + 1
    return (blocks + torch.minimum(blocks, torch.full_like(blocks, n_splits)) + 2).double() * 2.0 ** -24


def judge_graded(got, ref, allow):
    """got [B, nq, H, 128] bf16 against expected_graded()'s ref: got == bf16(ref); the adjacent pattern on ref's side only where ref lies
    within allow |ref| of the rounding boundary, and (Verdict.ok) for at most 0.1 % of the case's elements.  Every element is judged."""
    e, nb, dist = bf16_neighbourhood(ref)
    gd = got.double()
    eq = gd == e
    allowed = (~eq) & (gd == nb) & (dist <= allow[:, :, None, None] * ref.abs())
    ok = eq | allowed
    return Verdict((~ok).any(-1).any(-1), int((~ok).sum()), int(allowed.sum()), 0, got.numel())


def zone_share(ref, allow):
    """The share of a case's elements whose ref lies inside its allowance zone (a condition on the INPUTS)."""
    _, _, dist = bf16_neighbourhood(ref)
    return float(((dist <= allow[:, :, None, None] * ref.abs()) & (ref != 0)).sum()) / ref.numel()


def old_pin_count(got, ref):
    """Elements the tolerance tests' pin |err| <= 2^-8 |ref| + 2e-2 would flag."""
    return int(((got.double() - ref).abs() > 2.0 ** -8 * ref.abs() + 2e-2).sum())


def stream_partials_expected(c, positions, n_splits):
    """FLAT decode cases: the exact per-split partials of attn_decode_stream_kernel -- split s takes blocks s, s + n_splits, ...; m is
    the split's largest exponent, l = sum 2^(ex - m), part_o[d] = sum 2^(ex - m) v[d] (UNNORMALISED, relative to the split's own m); an
    empty split holds (-inf, 0, 0).  Every number is exact in fp32.  -> part_o [B, H, n_splits, 128], part_ml [B, H, n_splits, 2] fp32"""
    B, H = len(positions), c["v"].shape[2]
    po = torch.zeros(B, H, n_splits, HD, dtype=torch.float64)
    pml = torch.zeros(B, H, n_splits, 2, dtype=torch.float64)
    pml[..., 0] = float("-inf")
    one = torch.ones((), dtype=torch.float64)
    for b, p in enumerate(positions):
        ex = (int(c["mu"][b, 0]) * c["e"][b, :p + 1]).cpu()
        blk = torch.arange(p + 1) // 64
        vb = c["v"][b, :p + 1].double().cpu()
        for s in range(min(n_splits, int(blk.max()) + 1)):
            mine = blk % n_splits == s
            m = ex[mine].max()
            w = torch.ldexp(one, (ex[mine] - m).to(torch.int32))
            pml[b, :, s, 0], pml[b, :, s, 1] = float(m), w.sum()
            po[b, :, s] = torch.einsum("j,jhd->hd", w, vb[mine])
    return po.float(), pml.float()


# ------------------------------------------------------------------------------------------------ the stream kernel + combine in plain torch
def combine_tail_splits(n_splits):
    """The splits that attn_decode_combine_kernel's TAIL loop handles (group g = s mod 4 walks s = g, g + 4, ...; eight per trip while
    s + 28 < n_splits)."""
    out = []
    for g in range(4):
        s = g
        while s + 28 < n_splits:
            s += 32
        out += list(range(s, n_splits, 4))
    return sorted(out)


def emulate_stream(q, k, v, n_splits, c=1.0, defect=None):
    """fp32 emulation of attn_decode_stream_kernel + attn_decode_combine_kernel for one (batch row, head): q [128], k / v [n_keys, 128]
    bf16 -> (o [128] bf16, part_o [n_splits, 128], part_ml [n_splits, 2]).  32-key halves, a running maximum per split, alpha = 2^(m_old
    - m_new); the combine weights split s by 2^(m_s - M).  defect: a wrong arithmetic (tests/test_attn_graded_host.py)."""
    n = k.shape[0]
    sc_all = (k.double() @ q.double()).float() * torch.tensor(c, dtype=torch.float32)
    vf = v.float()
    nblk = (n + 63) // 64
    part_o = torch.zeros(n_splits, HD)
    part_ml = torch.zeros(n_splits, 2)
    ninf = torch.tensor(float("-inf"))
    for s in range(n_splits):
        m, l, o = ninf, torch.zeros(()), torch.zeros(HD)
        for blk in range(s, nblk, n_splits):
            for k0 in (64 * blk, 64 * blk + 32):
                if k0 >= n:
                    continue
                sc = sc_all[k0:k0 + 32]
                m_new = torch.maximum(m, sc.max())
                alpha = torch.exp2(m - m_new)
                a_l = a_o = alpha * (1 + 2.0 ** -10) if defect == "alpha_err" else alpha
                if defect == "alpha_l_only":
                    a_o = torch.ones(())
                if defect == "alpha_o_only":
                    a_l = torch.ones(())
                pw = torch.exp2(sc - m_new)
                if defect in ("skip8", "skip12"):
                    pw = torch.where(sc < sc.max() - float(defect[4:]), torch.zeros_like(pw), pw)
                l = l * a_l + pw.sum()
                o = o * a_o + pw @ vf[k0:k0 + 32]
                m = m_new
        part_o[s], part_ml[s, 0], part_ml[s, 1] = o, m, l
    ms = part_ml[:, 0]
    M = ms.max()
    mw = torch.roll(ms, -1) if defect == "combine_m_next" else ms
    w = torch.where(ms == float("-inf"), torch.zeros_like(ms), torch.exp2(torch.where(mw == float("-inf"), M, mw) - M))
    if defect == "tail_unweighted":
        w[combine_tail_splits(n_splits)] = 1.0
    L = (part_ml[:, 1] * w).sum()
    acc = (part_o * w[:, None]).sum(0)
    return (acc / L if L > 0 else torch.zeros(HD)).to(BF), part_o, part_ml


# ------------------------------------------------------------------------------------------------ G cases (shared by the CPU and the GPU module)
G_VARIANTS = (None, "N", "W1", "W2")                                     # flat + the three stair lists
G_W64 = [(W64_SHAPES[n], 3, 2) for n in (0, 3, 4, 6, 8)] + [(W64_SHAPES[0], 1, 8), (W64_SHAPES[6], 1, 8)]
G_PIPE = PIPE_SHAPES[:3]
G_QB128 = [(1, 199, 0), (37, 163, 0), (64, 136, 0), (128, 72, 0), (128, 63, 0)]      # Tk 200 (the last: 191)
G_QB128_LONG = (128, 1921, 0)                                            # Tk 2,049: flat only
G_PREFIX = [(P, Tq) for P in (64, 320) for Tq in (129, 321)]
G_DECODE_STAIR = [p for p in DECODE_POSITIONS if p <= 639] + [299, 555, 639]         # + three rows that reach the later levels
G_DECODE_SPLITS = [1, 4, 8, 40, None]


def graded_cuts(P=0):
    """The prefix cases put a cut on the P - 1 | P seam: 64 is one; for 320 the cut at 300 moves there (still a rise or drop >= 30)."""
    return tuple(P if (t == 300 and P == 320) else t for t in G_CUTS)


def graded_prefill(shape, B, H, dims, stair, device="cpu", P=0):
    Tq, q_pos0, dTk = shape
    Tk = q_pos0 + Tq + dTk
    win = G_WIN_STAIR if stair else graded_win(Tk)
    return build_graded(B, H, Tq, q_pos0, Tk, dims, win, stair, device, cuts=graded_cuts(P), shared_prefix=P)


def graded_decode(positions, H, dims, stair, device="cpu"):
    Tk = max(positions) + 1
    win = G_WIN_STAIR if stair else graded_win(Tk)
    return build_graded(len(positions), H, 1, 0, Tk, dims, win, stair, device, mult=decode_mult(positions, Tk, device), row_mu=True)
