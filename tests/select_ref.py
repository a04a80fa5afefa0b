"""TEST INFRASTRUCTURE (never imported by the product): input constructors, predictions and bounds for the two kernels that SELECT and
REDUCE -- the seeded device sampler (csrc/sample.hip) and the masked row pooling (csrc/pool.hip) -- in the style of tests/rowlocal_ref.py.
Everything here is eager torch / numpy; no kernel of libevo_mi355x.so is called.  tests/test_select_ref_host.py pins the predictions to
the written specification (evo_amd/sh/sample.py: sample_seeded) and to fp64 torch on the CPU; tests/test_gpu_sample_regimes.py and
tests/test_gpu_pool_exact.py use them as the yardstick.

1. FLAT rows.  With temperature 2^40 and logits inside +-64 every kept token's expf((v - v0) / T) is exactly 1.0f ((v - v0) / T is above
   -1.2e-10, half an ulp below 1 is 3e-8), so the kernel's prefix sums are the integers 1 .. n, Z = n, and the drawn token is
   order[floor(u n)]: order = "descending logit, ascending id", n = the size of the kept set, u = seeded_uniform(seed, stream, count).
   Tokens are compared for EQUALITY.  A row is left out only when u n lies within 2^-12 of an integer (the rounding of the fp32 target
   (float)(u Z) and a device expf that is one ulp off); the share is 2^-11 in expectation and capped at 0.5 % per launch.  Wherever
   top_p is active it is float32(0.381966): n (1 - p) is then at least 1.18e-3 from an integer for every n <= 512 (cut_distance), 40
   times the fp32 rounding of the kernel's threshold at n = 512, so no row is left out for the cut.
2. Non-flat extremes (extreme_cases): judged by tests/test_gpu_sample.py's own accept() / undecidable().
3. Pooling on bf16 integers in [-8, 8]: column sums of up to 3,000 rows stay below 2^24, so fp32 sums are exact in ANY order and the
   kernel's output is predictable to the bit (mode last, mean over 2^k rows) or to the two roundings of `* (1.0f / (float)n)`.
4. Pooling with the fused norm: a per-element bound that counts the fp32 additions on the longest path of the documented order.
"""
import functools

import numpy as np
import torch

from evo_amd.sh import sample as H

V = 512
NEG_INF = float("-inf")

# =========================================================================================== 1. sampler: flat rows
FLAT_T = 2.0 ** 40
P_CUT = float(np.float32(0.381966))          # 1.0f - p = 0.6180340052
U_MARGIN = 2.0 ** -12                        # a row is left out when u n is this close to an integer
FLAT_SEED = 20251
U_CAP = 0.005                                # ... and at most this share of a launch may be
CUT_MARGIN = 1.18e-3
TOP_KS = (0, 2, 3, 8, 9, 64, 65, 257, 511, 512, 513, 2 ** 31 - 1, -1)
ALL_KS = TOP_KS + (1,)                       # greedy rows interleaved with the others
TOP_PS = (0.0, 1.0, P_CUT)
A_ID = 65                                    # 'A': allowed by every mask below and finite in every row
MASKS = ("none", "acgt", "one", "m509")
M509_OUT = (0, 300, 511)
KINDS = ("int6", "int6", "int6", "int6", "int6", "int2", "int1", "const", "asc", "desc", "bitrev", "shuf", "ninf_int", "ninf_shuf",
         "ninf_const", "ninf_int1")
NINF_COUNTS = (1, 100, 511)
SUBNORMAL = 2.0 ** -130                      # a bf16 subnormal (8 x 2^-133)


def flat_mask(name):
    """bool [512] or None: "none", "acgt" (the four nucleotides), "one" (token 'A' alone), "m509" (all but three tokens)."""
    if name == "none":
        return None
    if name == "acgt":
        from evo_amd.tokenizer import CharLevelTokenizer
        return H.allowed_mask(CharLevelTokenizer(V), "ACGT")
    m = torch.zeros(V, dtype=torch.bool)
    if name == "one":
        m[A_ID] = True
    else:
        assert name == "m509", name
        m[:] = True
        m[list(M509_OUT)] = False
    return m


def _bf16_candidates():
    """Every 16th finite nonzero bf16 value inside +-64 (negatives and subnormals among them) except SUBNORMAL itself, as fp32."""
    bits = torch.arange(65536, dtype=torch.int32)
    e = (bits >> 7) & 0xff
    bits = bits[(e < 133) & ((bits & 0x7fff) != 0)]
    vals = bits.to(torch.int16).view(torch.bfloat16).float()[::16]
    return vals[vals != SUBNORMAL]


def bit_reverse9(i):
    r = torch.zeros_like(i)
    for b in range(9):
        r |= ((i >> b) & 1) << (8 - b)
    return r


def _distinct_rows(n, g):
    """[n, 512] fp32, ascending: 509 distinct candidates, SUBNORMAL, -0 and +0 (one value, two tokens) per row."""
    cand = _bf16_candidates()
    pick = torch.rand(n, cand.numel(), generator=g).argsort(dim=1)[:, :V - 3]
    rows = torch.cat([cand[pick], torch.full((n, 1), SUBNORMAL), torch.full((n, 1), -0.0), torch.zeros(n, 1)], dim=1)
    return torch.sort(rows, dim=1, stable=True)[0]


@functools.lru_cache(maxsize=None)
def flat_case(S=8192, seed=0):
    """The launch of section 1: rows [S, 512] fp32 holding bf16 values (row r is of kind KINDS[r % 16]) and heterogeneous per-row
    top_k / top_p, temperature 2^40 (0.7 on the greedy rows, which ignore it), stream 3 r + 1, count 5 r mod 1000.
    Kinds: integers in [-6, 6] / [-2, 2] / [-1, 1] (ties at every cut); a constant row; 512 distinct-valued bf16 entries (-0 and +0
    count as one value) ascending, descending, in bit-reversed order and shuffled -- the adversarial inputs of a bitonic network;
    ninf_*: 1, 100 or 511 entries already -inf (token 'A' always stays finite, so no mask below empties a row)."""
    g = torch.Generator().manual_seed(7700 + seed)
    r = torch.arange(S)
    kind = r % 16
    rows = torch.randint(-6, 7, (S, V), generator=g).float()
    small = torch.randint(-2, 3, (S, V), generator=g).float()
    sel = kind == KINDS.index("int2")
    rows[sel] = small[sel]
    sel = (kind == KINDS.index("int1")) | (kind == KINDS.index("ninf_int1"))
    rows[sel] = small[sel].clamp(-1, 1)
    sel = (kind == KINDS.index("const")) | (kind == KINDS.index("ninf_const"))
    rows[sel] = (((r[sel] // 16) % 13) - 6).float()[:, None].expand(-1, V)
    for name in ("asc", "desc", "bitrev", "shuf", "ninf_shuf"):
        sel = torch.nonzero(kind == KINDS.index(name)).flatten()
        d = _distinct_rows(sel.numel(), g)
        if name == "desc":
            d = d.flip(1)
        elif name == "bitrev":
            d = d[:, bit_reverse9(torch.arange(V))]
        elif name in ("shuf", "ninf_shuf"):
            d = d.gather(1, torch.rand(sel.numel(), V, generator=g).argsort(dim=1))
        rows[sel] = d
    # entries already -inf: the first m ids of a per-row shuffle that never names A_ID
    sel = torch.nonzero(kind >= KINDS.index("ninf_int")).flatten()
    others = torch.tensor([i for i in range(V) if i != A_ID])
    perm = others[torch.rand(sel.numel(), V - 1, generator=g).argsort(dim=1)]
    m = torch.tensor(NINF_COUNTS)[(sel // 16 + sel) % 3]
    drop = torch.arange(V - 1)[None, :] < m[:, None]
    hole = torch.zeros(sel.numel(), V, dtype=torch.bool).scatter_(1, perm, drop)
    rows[sel] = rows[sel].masked_fill(hole, NEG_INF)
    assert torch.equal(rows.bfloat16().float(), rows)                      # every entry is a bf16 value
    top_k = torch.tensor(ALL_KS, dtype=torch.int64)[torch.randint(0, len(ALL_KS), (S,), generator=g)]
    top_p = torch.tensor(TOP_PS, dtype=torch.float32)[torch.randint(0, len(TOP_PS), (S,), generator=g)]
    temperature = torch.where(top_k == 1, torch.tensor(0.7), torch.tensor(FLAT_T)).float()
    return dict(rows=rows, kind=kind, top_k=top_k.to(torch.int32), top_p=top_p, temperature=temperature,
                stream=r.to(torch.int64) * 3 + 1, count=(r.to(torch.int64) * 5) % 1000)


def cut_distance(q=None):
    """min over n = 1 .. 512 of the distance of n q from an integer; q defaults to 1 - P_CUT in fp64."""
    q = 1.0 - P_CUT if q is None else float(q)
    t = np.arange(1, V + 1, dtype=np.float64) * q
    d = np.abs(t - np.round(t))
    return float(d.min()), int(d.argmin()) + 1


def flat_order(rows, mask=None):
    """(order [S, 512], n_finite [S], sorted values [S, 512]): tokens by descending masked logit, ties by ascending id."""
    x = rows.detach().cpu().double()
    if mask is not None:
        x = x.masked_fill(~mask[None, :], NEG_INF)
    srt, order = torch.sort(x, dim=-1, descending=True, stable=True)      # (-0 == +0 for the comparison: one value)
    return order, (srt > NEG_INF).sum(-1), srt


def flat_kept(srt, n_finite, top_k, top_p):
    """n [S]: how many tokens of `order` a flat row keeps.  top_k in (1, 512): the finite logits >= the k-th largest (ties stay); any
    other top_k: the finite logits.  0 < top_p < 1: the ascending cumulative softmax of n equal terms is j / n, dropped while
    <= 1 - top_p: floor(n (1 - top_p)) tokens go."""
    k = top_k.long()
    kth = srt.gather(-1, (k.clamp(1, V) - 1)[:, None])
    n = torch.where((k > 1) & (k < V), torch.minimum(n_finite, (srt >= kth).sum(-1)), n_finite)
    p = top_p.double()
    cut = (p > 0) & (p < 1)
    return torch.where(cut, n - torch.floor(n.double() * (1.0 - p)).long(), n)


def flat_draw(order, n, top_k, seed, stream, count, index=None):
    """(token [S], left out [S] bool) of rows that keep the first n tokens of `order`: order[floor(u n)], position 0 on greedy rows.
    With `index` [S], row s of the launch is row index[s] of order / n / top_k (a launch that repeats its rows under other keys)."""
    if index is not None:
        n, top_k = n[index], top_k[index]
    S = n.shape[0]
    u = H.seeded_uniform(seed, np.broadcast_to(np.asarray(stream, dtype=np.int64), (S,)),
                         np.broadcast_to(np.asarray(count, dtype=np.int64), (S,)))
    t = torch.from_numpy(np.ascontiguousarray(u)) * n.double()
    greedy = top_k.cpu().long() == 1
    pos = torch.where(greedy, torch.zeros_like(n), torch.floor(t).long().clamp(max=V - 1))
    out = ((t - torch.round(t)).abs() <= U_MARGIN) & ~greedy
    tok = order[torch.arange(S) if index is None else index, pos]
    return tok, out


def flat_predict(rows, top_k, top_p, mask, seed, stream, count, order=None):
    """(token [S], left out [S] bool, n kept [S]) of a flat launch.  `order` = flat_order(rows, mask) when the caller has it."""
    order, n_fin, srt = flat_order(rows, mask) if order is None else order
    assert int(n_fin.min()) >= 1
    n = flat_kept(srt, n_fin, top_k.cpu(), top_p.cpu())
    tok, out = flat_draw(order, n, top_k, seed, stream, count)
    return tok, out, torch.where(top_k.cpu().long() == 1, torch.ones_like(n), n)


@functools.lru_cache(maxsize=None)
def flat_expected(mask_name, seed=FLAT_SEED):
    """flat_predict of flat_case() under one of MASKS, computed once per session: (token, left out, n kept, (order, n_finite, sorted))."""
    c = flat_case()
    od = flat_order(c["rows"], flat_mask(mask_name))
    tok, out, n = flat_predict(c["rows"], c["top_k"], c["top_p"], None, seed, c["stream"].numpy(), c["count"].numpy(), order=od)
    return tok, out, n, od


# 64-bit keying (section 2 of the module): j is the row index
SEEDS64 = (5, 2 ** 32 + 5, 2 ** 63 + 12345, -1)
STREAMS64 = {"j": lambda j: j, "2^32+j": lambda j: 2 ** 32 + j, "-1-j": lambda j: -1 - j, "2^62+j": lambda j: 2 ** 62 + j}
COUNTS64 = {"j": lambda j: j, "2^32+j": lambda j: 2 ** 32 + j, "2^40": lambda j: np.full_like(j, 2 ** 40)}


def low32(x):
    """The value a kernel would see had it dropped the high word (as a non-negative integer / int64 array)."""
    return (int(x) & 0xFFFFFFFF) if isinstance(x, int) else (np.asarray(x, dtype=np.int64) & np.int64(0xFFFFFFFF))


# =========================================================================================== 2. sampler: non-flat extremes
def _randn3(n, seed):
    return (torch.randn(n, V, generator=torch.Generator().manual_seed(seed)) * 3.0).bfloat16()


@functools.lru_cache(maxsize=None)
def extreme_rows(name, n=4096):
    """randn3: bf16 N(0, 9).  wide: f32 uniform over +-3e4 (most exp terms underflow to 0 or to subnormals) with three more entries
    0.5, 1.25 and 2 above the row's maximum, so that the draw is not a foregone conclusion.  spike: randn3 with one entry at +60.
    top2: randn3 with the row's maximum written over its second-largest entry (the two largest logits are equal)."""
    g = torch.Generator().manual_seed(len(name) * 1000 + n)
    if name == "randn3":
        return _randn3(n, 41)
    if name == "wide":
        x = (torch.rand(n, V, generator=g) * 2 - 1) * 3.0e4
        top = x.max(-1)[0]
        at = torch.rand(n, V, generator=g).argsort(dim=1)[:, :3]
        x.scatter_(1, at, top[:, None] + torch.tensor([0.5, 1.25, 2.0])[None, :])
        return x
    if name == "spike":
        x = _randn3(n, 42)
        x.scatter_(1, torch.randint(0, V, (n, 1), generator=g), 60.0)
        return x
    assert name == "top2", name
    x = _randn3(n, 43)
    top2 = x.float().topk(2, dim=-1)
    x.scatter_(1, top2[1][:, 1:2], top2[0][:, 0:1].bfloat16())
    return x


# (name of the rows, f32 launch, [(top_k, top_p, temperature)], compare logprob_out).  top_p < 1 only up to T = 1.2: at T = 30 the
# ascending CDF steps are ~2e-3 apart and too many rows would be undecidable -- that regime is the flat rows' (exact) business.
EXTREME_CASES = (
    ("randn3", False, ((0, 1.0, 0.05), (50, 1.0, 0.05), (0, 1.0, 30.0), (50, 1.0, 30.0), (50, 0.7, 0.0), (4, 0.9, -1.0)), False),
    ("wide", True, ((0, 1.0, 1.0), (0, 0.9, 1.0), (8, 1.0, 30.0)), True),
    ("spike", False, ((0, 0.9, 1.0), (0, 1.0, 30.0), (50, 0.7, 0.05)), True),
    ("top2", False, ((50, 0.7, 1.0), (2, 1.0, 0.7), (4, 0.9, 1.2), (2, 1.0, 30.0)), False),
)
EXTREME_SEED = 31337
UNDECIDABLE_CAP = 0.04


def extreme_keys(n):
    j = np.arange(n, dtype=np.int64)
    return j * 7 + 3, (j * 11) % 777


# =========================================================================================== 3. pooling: exact sums
POOL_WIDTHS = (8, 264, 520, 1032, 2056, 4096)       # nvec 1, 33, 65, 129, 257, 512 -> pool_strip_kernel<1 | 1 | 2 | 4 | 8 | 8>
POOL_LENGTHS = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65, 1000, 2048, 3000)
OUTSIDE = 1.0e4                                     # rows outside every range


def pool_plan_nv(D):
    """The register plan evo_pool_rows_bf16 picks: 16-byte vectors per lane."""
    nvec = D // 8
    return 1 if nvec <= 64 else 2 if nvec <= 128 else 4 if nvec <= 256 else 8


def pool_int_rows(M, D, device="cpu"):
    """[M, D] bf16 integers in [-8, 8], a hash of (row, column): every row differs (asserted on the host for the shapes in use)."""
    r = torch.arange(M, dtype=torch.int64, device=device)[:, None]
    c = torch.arange(D, dtype=torch.int64, device=device)[None, :]
    h = (r * 2654435761 + c * 40503 + (r >> 3) * (c + 1) * 97 + (r * r) * 31) & 0xFFFFFFFF
    h = (h ^ (h >> 15)) * 2246822519 & 0xFFFFFFFF
    return (((h >> 11) % 17) - 8).to(torch.bfloat16)


def ragged_layout(lengths, gap=3):
    """(ranges, M, inside [M] bool): the first range starts at row 0, `gap` rows that belong to no range lie between two ranges, the last
    range ends at row M - 1."""
    ranges, a = [], 0
    for n in lengths:
        ranges.append((a, n))
        a += n + gap
    M = a - gap
    inside = torch.zeros(M, dtype=torch.bool)
    for a, n in ranges:
        inside[a:a + n] = True
    return ranges, M, inside


def pool_strips(B, longest, workgroups=None):
    """n_strips as HipOps.pool_rows picks it in mode "mean" (`longest` = the longest range of a list, M for a tensor of ranges)."""
    if workgroups is None:
        from evo_amd.ops import HipOps
        workgroups = HipOps.POOL_WORKGROUPS
    return max(1, min(-(-workgroups // B), -(-longest // 16)))


def pool_chunk(n, n_strips):
    return -(-n // n_strips)


def pool_adds(n, n_strips):
    """fp32 additions on the longest path of a pooled mean, in the documented order: ceil(chunk / 4) rows in a wave, 2 merges of the 4
    waves, ceil(n_strips / 16) slabs in a wave of the finish kernel, 15 merges of its 16 waves."""
    return -(-pool_chunk(n, n_strips) // 4) + 2 + -(-n_strips // 16) + 15


def pool_exact_ref(x, ranges, mode):
    """fp64 [B, D]: the last row, or (exact sum) / n, of each range of an integer-valued x."""
    outs = []
    for a, n in ranges:
        outs.append(x[a + n - 1].double() if mode == "last" else x[a:a + n].double().sum(0) / n)
    return torch.stack(outs)


def is_pow2(n):
    return n & (n - 1) == 0


# =========================================================================================== 4. pooling with the fused norm
NORM_WIDTHS = (264, 1032, 4096)
NORM_LENGTHS = (1, 5, 17, 64, 1000, 3000)
RSTD_ERR = 2e-6                                     # the project's pin of the fp32 1 / (rms + eps) factor (PARITY rows 11a, 24c)


def pool_norm_rows(M, D, seed=0, device="cpu"):
    """x [M, D] bf16 and scale [D] bf16.  Row r: randn * 1.5 + 0.5, times 2^40 (r % 5 == 1) or 2^-40 (r % 5 == 2), channel D // 3 times
    10^4 (r % 5 == 3), zero (r % 25 == 4)."""
    g = torch.Generator().manual_seed(900 + seed + D)
    x = (torch.randn(M, D, generator=g) * 1.5 + 0.5).double()
    r = torch.arange(M)
    x[r % 5 == 1] *= 2.0 ** 40
    x[r % 5 == 2] *= 2.0 ** -40
    x[r % 5 == 3, D // 3] *= 1.0e4
    x[r % 25 == 4] = 0
    scale = (torch.rand(D, generator=g) + 0.5).to(torch.bfloat16)
    return x.to(torch.bfloat16).to(device), scale.to(device)


def pool_norm_ref(x, ranges, scale, eps):
    """(ref [B, D], A [B, D]) in fp64: ref = scale (1 / n) sum_r f(x_r), A = abs(scale) (1 / n) sum_r abs(f(x_r)), with
    f(x) = x / (||x||_2 D^-1/2 + eps) -- the engine's RMSNorm, eps outside the root."""
    D = x.shape[1]
    sc = scale.double()
    ref, mag = [], []
    for a, n in ranges:
        r = x[a:a + n].double()
        f = r / (torch.linalg.vector_norm(r, dim=1, keepdim=True) * D ** -0.5 + eps)
        ref.append(f.sum(0) / n * sc)
        mag.append(f.abs().sum(0) / n * sc.abs())
    return torch.stack(ref), torch.stack(mag)


def pool_norm_bound(A, n, n_strips):
    """((L + 4) 2^-24 + 2e-6) A: L = pool_adds roundings of the sums, 4 for the fma, the two of `* (1.0f / n)` and the scale; 2e-6 for
    each row's factor."""
    return ((pool_adds(n, n_strips) + 4) * 2.0 ** -24 + RSTD_ERR) * A
