"""TEST INFRASTRUCTURE (never imported by the product): EXACT inputs, the reference and a plain-torch emulation for the decode attention
on the FP8 (e4m3fn) KV cache (csrc/kv_fp8.hip, attn_decode_fp8_kernel), as tests/attn_exact.py is for the bf16 attention kernels.
Everything here is eager torch on whatever device is asked for; no kernel of libevo_mi355x.so is called.
tests/test_kv_fp8_exact_host.py pins this module on the CPU, tests/test_gpu_kv_fp8_exact.py uses it.  The closed forms, the judge, the
decode multiplicities, the split counts and the hash are attn_exact's (`expected`, `judge`, `decode_mult`, `stream_split_counts`, `mix31`).

A cache is built DIRECTLY as (bytes, scale) in the Fp8KV layout -- data [B + 1, cap, 2, H, 128] uint8, scale [B + 1, 2, H, cap] f32: these
are the kernel's inputs, and the kernel does not care whether a pair is the one the quantising rule would have chosen.  Every dequantised
value byte * scale is exact (`f8_bytes` asserts it), so every softmax weight is exactly 1 or 0 as in attn_exact.

Scores.  e4m3 has 4 significant bits, so a key number is written in base 16: digit i (0 .. 15) in dim dims[i], q = G 16^i there (3 dims up
to 4,096 keys, 4 up to 65,536, 5 beyond).  Every partial sum of a score is a multiple of G = 2,048 below 2^24 G (times ONE power of two per
key in the non-canonical storage): exact in fp32 in any order.  Plain form (c = 0.12753) and PRE both apply to the same data.  `DIMSETS`
rotate between cases so that each of the eight 16-byte chunks of a row (the kernel's dc) carries a digit in some case.
  U    q = 0; K is arbitrary finite bytes with arbitrary power-of-two scales.  V[j, d] is nonzero only at d = j mod 128, its byte is 1.0
       (alt: -1.0 where (j div 128) is odd) and its V scale s_bh 2^(hash(b, h, j) mod 4): the output is a small integer times a power of two
       over the key count.  One key dropped or doubled, or given its neighbour's V scale, moves an output.
  D    key j has number j, q positive: the last visible key wins.  D': q negated, key 0 wins.  V bytes are hashed finite e4m3 patterns
       (0x7f / 0xff and -0 excluded; both signs, +0 and subnormals included), the V scale is 2^e, e hashed in [-20, 20] per (b, h, key): the
       output is bf16(byte * scale) of the winner, exact.
  S    number 0 except planted keys t_1 < t_2 < ... with numbers 1, 2, ...: D-type V rows on the planted keys, U-type rows elsewhere.
  non-canonical K storage (D, D', S): key j's digits are stored as digit 2^-t with K scale 2^t, t hashed in [-3, 3] per (b, h, key).  The
       dequantised key is unchanged; a K scale taken from another key, head or plane moves that key's level by a power of two.
Canaries.  Keys behind a row's position but inside its last 32-key half hold byte 0x7e (448) with scale 2^100 in both planes (finite: a
masked weight is an exact 0).  Everything further behind, and the spare batch row, is byte 0x7f (NaN) with NaN scales.

`emulate` walks the cache the way the kernel does, in fp32: lane = (ks, dc), 16-element partial dots and their three-step lane sum, score =
dot x K scale x scale_log2, the half-by-half running (m, l, O) per key group with the probability multiplied by the V scale once, the ring of
three buffers with its load guards, the interleaved block-to-split map, the dropped second half, the combine.  `defect` switches in ONE
wrong statement (DEFECTS).  Every product of these designs is exact in fp32, so a * b + c below rounds once, as the kernel's fma does.
"""
import math

import torch

import attn_exact as X
from attn_exact import ALLOW_REL, ALLOW_SHARE, G, HD, decode_mult, expected, judge, mix31, stream_split_counts  # noqa: F401 (re-exported)

BF = torch.bfloat16
F8 = torch.float8_e4m3fn
NAN_BYTE, CANARY_BYTE = 0x7f, 0x7e
CANARY_SCALE = 2.0 ** 100
DIMSETS = ((0, 17, 34, 51, 68), (85, 102, 119, 15, 16), (127, 112, 96, 47, 40), (50, 70, 90, 5, 110))
assert {d // 16 for ds in DIMSETS for d in ds[:3]} == set(range(8))      # the three digits every case uses reach every chunk dc
T_RANGE = 3                                                              # non-canonical storage: t in [-3, 3]
E_RANGE = 20                                                             # D-type V scales: 2^e, e in [-20, 20]


def n_digits(n_keys):
    n = 3
    while 16 ** n < n_keys:
        n += 1
    return n


def f8_bytes(x):
    """An exactly representable float tensor -> its e4m3fn bit patterns (uint8)."""
    b = x.float().to(F8)
    assert torch.equal(b.float(), x.float()), "a value of an exact design is not an e4m3 value"
    return b.view(torch.uint8)


def f8_value(byts):
    return byts.view(F8).float()


def pow2(e):
    """2^e as f32 for an integer tensor e in [-126, 127]."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def _key_index(B, T, H, device):
    """[B, T, H] int64: a distinct number per (b, key, h) that does not depend on B, T or H."""
    b = torch.arange(B, dtype=torch.int64, device=device)[:, None, None]
    t = torch.arange(T, dtype=torch.int64, device=device)[None, :, None]
    h = torch.arange(H, dtype=torch.int64, device=device)[None, None, :]
    return (b * 64 + h) * (1 << 20) + t


def finite_bytes(z):
    """A hash -> every e4m3fn pattern but the two NaNs (0x7f, 0xff) and -0 (0x80: an accumulator that starts at +0 returns +0 for it)."""
    r = z % 253
    return (r + 2 * (r >= 0x7f).to(r.dtype)).to(torch.uint8)


# ------------------------------------------------------------------------------------------------ designs
def seams(n_keys, split_counts, own=True):
    """S: the keys the issue names -- 0 / 31 / 32 / 33 / 63 / 64 / 65, 64 n_splits -+ for every split count of the test, the last key of
    each split's first block (of the first 24 splits) and, with `own`, the row's own two: the first key of its last 32-key half and its
    last key."""
    ts = {0, 31, 32, 33, 63, 64, 65}
    if own:
        ts |= {n_keys - 1, (n_keys - 1) // 32 * 32}
    for ns in split_counts:
        ts |= {64 * ns - 1, 64 * ns}
    ts |= {64 * s + 63 for s in range(min(max(split_counts), 24))}
    return sorted(t for t in ts if 0 <= t < n_keys)


def planted_for(positions, split_counts):
    """One ascending list per batch row.  Even rows plant everything: their last key wins.  Odd rows plant neither their own two keys nor
    key 0: an interior seam wins over the uniform tail behind it, and rows in front of key 31 return the U mean."""
    return [seams(p + 1, split_counts, own=b % 2 == 0)[b % 2:] for b, p in enumerate(positions)]


def build(design, positions, H, dims, device="cpu", noncanon=False, alt=False, planted=None, Tk=None):
    """The CLEAN case (no canaries, no poison): q [B, 1, H, 128] bf16, kb / vb [B, Tk, H, 128] uint8, ks / vs [B, Tk, H] f32, lev [B, Tk]
    int64 (a key's level in units of G), mult [B, 1, Tk], v [B, Tk, H, 128] bf16 -- the dequantised values, for `expected`."""
    B = len(positions)
    Tk = max(positions) + 1 if Tk is None else Tk
    nd = n_digits(Tk)
    dims = tuple(dims[:nd])
    assert len(dims) == nd, "this key count needs more digit dims"
    j = torch.arange(Tk, dtype=torch.int64, device=device)
    kidx = _key_index(B, Tk, H, device)
    q = torch.zeros(B, 1, H, HD, dtype=torch.float32, device=device)
    if design == "U":
        assert not noncanon
        kb = finite_bytes(mix31(X._index(B, Tk, H, device), 71))
        ks = pow2(mix31(kidx, 72) % (2 * T_RANGE + 1) - T_RANGE)
        lev = torch.zeros(B, Tk, dtype=torch.int64, device=device)
    else:
        if design in ("D", "D'"):
            num = j[None, :].expand(B, Tk).contiguous()
            lev = num if design == "D" else -num
        elif design == "S":
            num = torch.zeros(B, Tk, dtype=torch.int64, device=device)
            for b in range(B):
                ts = planted[b]
                assert ts == sorted(set(ts)) and all(0 <= t < Tk for t in ts) and len(ts) < 16 ** nd
                if ts:
                    num[b, torch.tensor(ts, dtype=torch.int64, device=device)] = torch.arange(1, len(ts) + 1, dtype=torch.int64, device=device)
            lev = num
        else:
            raise ValueError(design)
        t = mix31(kidx, 73) % (2 * T_RANGE + 1) - T_RANGE if noncanon else torch.zeros_like(kidx)
        ks = pow2(t)
        kval = torch.zeros(B, Tk, H, HD, dtype=torch.float32, device=device)
        for i, d in enumerate(dims):
            kval[..., d] = ((num // 16 ** i) % 16).float()[:, :, None] * pow2(-t)
            q[..., d] = (-1.0 if design == "D'" else 1.0) * G * 16.0 ** i
        kb = f8_bytes(kval)
        del kval
    # values
    one = (j % HD)[:, None] == torch.arange(HD, dtype=torch.int64, device=device)[None, :]
    hist_b = torch.where(one, 0x38, 0).to(torch.uint8)                                        # 1.0
    if alt:
        hist_b = torch.where(one & (((j // HD) % 2) == 1)[:, None], 0xb8, hist_b.to(torch.int64)).to(torch.uint8)      # -1.0
    hist_s = (X.head_factor(B, H, device).float()[:, :, :, 0] * pow2(mix31(kidx, 74) % 4))     # [B, Tk, H]
    if design == "U":
        vb, vs = hist_b[None, :, None, :].expand(B, Tk, H, HD).contiguous(), hist_s
    else:
        vb = finite_bytes(mix31(X._index(B, Tk, H, device), 75))
        vs = pow2(mix31(kidx, 76) % (2 * E_RANGE + 1) - E_RANGE)
        if design == "S":
            isp = (num > 0)[:, :, None]
            vb = torch.where(isp[..., None], vb, hist_b[None, :, None, :])
            vs = torch.where(isp, vs, hist_s)
    vf = f8_value(vb) * vs[..., None]
    v = vf.to(BF)
    assert torch.equal(v.float(), vf), "a dequantised value is not a bf16 value"
    return {"design": design, "q": q.to(BF), "kb": kb, "ks": ks, "vb": vb, "vs": vs, "lev": lev, "v": v, "positions": list(positions), "dims": dims,
            "mult": decode_mult(positions, Tk, device), "planted": planted, "noncanon": noncanon}


def dequantised_keys(c):
    """[B, Tk, H, 128] fp32, exact."""
    return f8_value(c["kb"]) * c["ks"][..., None]


def pack(c, cap=None, n_keys=None):
    """The clean case -> (data [B + 1, cap, 2, H, 128] uint8, scale [B + 1, 2, H, cap] f32) with row b's keys 0 .. positions[b] (n_keys:
    the scalar form -- every row holds keys 0 .. n_keys - 1), canaries up to the end of the row's last 32-key half, NaN behind."""
    kb, vb, ks, vs = c["kb"], c["vb"], c["ks"], c["vs"]
    B, Tk, H, _ = kb.shape
    cap = Tk if cap is None else cap
    dev = kb.device
    n = torch.tensor([p + 1 for p in c["positions"]] if n_keys is None else [n_keys] * B, dtype=torch.int64, device=dev)[:, None]
    j = torch.arange(cap, dtype=torch.int64, device=dev)[None, :]
    vis, can = j < n, (j >= n) & (j < (n + 31) // 32 * 32)
    data = torch.full((B + 1, cap, 2, H, HD), NAN_BYTE, dtype=torch.uint8, device=dev)
    scale = torch.full((B + 1, 2, H, cap), float("nan"), dtype=torch.float32, device=dev)
    data[:B][can] = CANARY_BYTE
    m = min(Tk, cap)
    for w, (byts, sc) in enumerate(((kb, ks), (vb, vs))):
        data[:B, :m, w] = torch.where(vis[:, :m, None, None], byts[:, :m], data[:B, :m, w])
        plane = torch.where(can[:, None, :], torch.full_like(scale[:B, w], CANARY_SCALE), scale[:B, w])
        plane[:, :, :m] = torch.where(vis[:, None, :m], sc[:, :m].permute(0, 2, 1), plane[:, :, :m])
        scale[:B, w] = plane
    return data, scale


# ------------------------------------------------------------------------------------------------ the kernel's walk, in torch
# name -> what the wrong statement is.  A defect is a name or (name, argument).
DEFECTS = {
    "kscale": "the K scale of key j + arg (lane 8 i + ks + arg of the scale request)",
    "vscale": "the V scale of key j + arg (lane 32 + 8 i + ks + arg)",
    "kforv": "the K scale used for V: lane 8 i + ks instead of 32 + 8 i + ks",
    "head": "the scales of head h ^ 1",
    "planes": "the scale planes swapped (lanes 0-31 fetch the V plane)",
    "le": "the ragged mask < changed to <=: the clamped last key is counted twice",
    "keep": "the second half beyond the keys kept (no --n_my)",
    "ring": "the third half of a trip reduced from kB / vB / sB",
    "skip": "the wave's last half not reduced when n_my mod 3 == arg",
    "map": "a contiguous block-to-split map: split s takes ceil(nblk / n_splits) consecutive blocks",
    "noalpha": "l_run not rescaled by alpha",
    "chunk": "chunk dc read as dc ^ 1 (K and V)",
}
ALL_DEFECTS = [("kscale", 1), ("kscale", -1), ("vscale", 1), ("vscale", -1), "kforv", "head", "planes", "le", "keep", "ring", ("skip", 0),
               ("skip", 1), ("skip", 2), "map", "noalpha", "chunk"]


def defect_id(d):
    return d if isinstance(d, str) else f"{d[0]}{d[1]:+d}"


def _tree8(x, dim):
    """((x0 + x1) + (x2 + x3)) + ((x4 + x5) + (x6 + x7)) along `dim` of size 8: the XOR1 / XOR2 / HALF_MIRROR lane sum of a key's eight
    chunks, and the xor 8 / 16 / 32 meeting of the eight key groups."""
    p = x.unflatten(dim, (4, 2))
    s = p.select(dim + 1, 0) + p.select(dim + 1, 1)
    s = s.unflatten(dim, (2, 2))
    s = s.select(dim + 1, 0) + s.select(dim + 1, 1)
    return s.select(dim, 0) + s.select(dim, 1)


def emulate(q, data, scale, positions, n_splits, pre, defect=None, n_keys=None):
    """q [B, 1, H, 128] bf16, (data, scale) as `pack` returns them, positions [B] (None: the scalar form with n_keys) ->
    (o [B, 1, H, 128] bf16, part_ml [B, H, n_splits, 2] f32): attn_decode_fp8_kernel + attn_decode_combine_kernel in fp32 torch."""
    name, arg = (defect, None) if defect is None or isinstance(defect, str) else defect
    assert name is None or name in DEFECTS
    dev = q.device
    B, _, H, _ = q.shape
    f32 = torch.float32
    ns = n_splits
    nk = (torch.tensor(positions, dtype=torch.int64, device=dev) + 1 if positions is not None
          else torch.full((B,), n_keys, dtype=torch.int64, device=dev))[:, None]                     # [B, 1]
    nblk, nhalf = (nk + 63) // 64, (nk + 31) // 32
    S = min(ns, int(nblk.max()))                                      # waves beyond own no block of any row: (-inf, 0, 0)
    s = torch.arange(S, dtype=torch.int64, device=dev)[None, :]       # [1, S]
    if name == "map":
        per = (nblk + ns - 1) // ns
        first = s * per
        nb_my = (torch.minimum(first + per, nblk) - first).clamp_min(0)
        half_of = lambda jh: 2 * (first + (jh >> 1)) + (jh & 1)       # noqa: E731
    else:
        nb_my = torch.where(s < nblk, (nblk - s + ns - 1) // ns, torch.zeros_like(nblk))
        half_of = lambda jh: 2 * (s + (jh >> 1) * ns) + (jh & 1)      # noqa: E731
    n_my = 2 * nb_my                                                  # [B, S]
    if name != "keep":
        n_my = n_my - ((n_my > 0) & (half_of(n_my - 1) >= nhalf)).to(torch.int64)
    c = torch.tensor(1.0, dtype=f32, device=dev) if pre else \
        torch.tensor(1.0 / math.sqrt(HD), dtype=f32, device=dev) * torch.tensor(1.4426950408889634, dtype=f32, device=dev)
    qf = q[:, 0].float()[:, None, None]                               # [B, 1, 1, H, 128]
    tokens = data[:B]
    if name == "chunk":
        tokens = tokens[..., torch.arange(HD, device=dev) ^ 16]
    sc_tok = scale[:B].permute(0, 3, 1, 2)                            # [B, cap, 2, H]
    if name == "head":
        sc_tok = sc_tok[..., torch.arange(H, device=dev) ^ 1]
    if name == "planes":
        sc_tok = sc_tok.flip(2)
    bi = torch.arange(B, device=dev)[:, None, None]
    lane = torch.arange(32, dtype=torch.int64, device=dev)
    k_lane = (lane + arg) % 64 if name == "kscale" else lane
    v_lane = (32 + lane + arg) % 64 if name == "vscale" else lane if name == "kforv" else 32 + lane
    ninf = torch.tensor(float("-inf"), dtype=f32, device=dev)
    m_run = torch.full((B, S, H), float("-inf"), dtype=f32, device=dev)
    l_run = torch.zeros(B, S, H, 8, dtype=f32, device=dev)            # per key group ks
    o_run = torch.zeros(B, S, H, 8, HD, dtype=f32, device=dev)

    def reduce_half(jh, buf, act):
        """Half number jh of every wave (mask and key numbers from jh) reduced from a buffer that holds the half it was LOADED with
        (buf [B, S]: the wave's half number at load time, -1: never loaded -> zeros); act [B, S]: the waves that take this step."""
        nonlocal m_run, l_run, o_run
        if name == "skip":
            act = act & ~((n_my - 1 == jh) & (n_my % 3 == arg))
        if not bool(act.any()):
            return
        loaded = (buf >= 0) & act
        key = half_of(buf.clamp_min(0))[..., None] * 32 + lane        # [B, S, 32]: load_half's clamp
        key = torch.minimum(key, nk[..., None] - 1).clamp_min(0)
        key = torch.where(loaded[..., None], key, torch.zeros_like(key))
        raw = tokens[bi, key]                                         # [B, S, 32, 2, H, 128]
        ld = loaded[:, :, None, None, None].to(f32)
        kf, vf = f8_value(raw[:, :, :, 0]) * ld, f8_value(raw[:, :, :, 1]) * ld
        st = sc_tok[bi, key]                                          # [B, S, 32, 2, H]
        lanes = torch.cat([st[:, :, :, 0], st[:, :, :, 1]], 2) * loaded[:, :, None, None].to(f32)      # the 64 lanes of the scale request
        s_k, s_v = lanes[:, :, k_lane], lanes[:, :, v_lane]           # [B, S, 32, H]
        # the 16-element partial dots (d0: even elements, d1: odd ones, in order), then the three-step lane sum
        prod = (kf * qf).unflatten(-1, (8, 16))
        d0 = torch.zeros_like(prod[..., 0])
        d1 = torch.zeros_like(d0)
        for e in range(0, 16, 2):
            d0 = d0 + prod[..., e]
            d1 = d1 + prod[..., e + 1]
        d = _tree8(d0 + d1, 4)                                        # [B, S, 32, H]
        kn = half_of(torch.full_like(n_my, jh))[..., None] * 32 + lane
        seen = kn <= nk[..., None] if name == "le" else kn < nk[..., None]
        sc = torch.where(seen[..., None], d * s_k * c, ninf)
        m_new = torch.maximum(m_run, sc.amax(2))
        alpha = torch.exp2(m_run - m_new)
        pw = torch.exp2(sc - m_new[:, :, None])                       # [B, S, 32, H]
        pv = pw * s_v
        l_new = l_run if name == "noalpha" else l_run * alpha[..., None]
        o_new = o_run * alpha[..., None, None]
        pw4, pv4 = pw.unflatten(2, (4, 8)), pv.unflatten(2, (4, 8))    # key 8 i + ks: [B, S, i, ks, H]
        vf4 = vf.unflatten(2, (4, 8))
        for i in range(4):
            l_new = l_new + pw4[:, :, i].permute(0, 1, 3, 2)
            o_new = o_new + (pv4[:, :, i, :, :, None] * vf4[:, :, i]).permute(0, 1, 3, 2, 4)
        a3 = act[..., None]
        m_run = torch.where(a3, m_new, m_run)
        l_run = torch.where(a3[..., None], l_new, l_run)
        o_run = torch.where(a3[..., None, None], o_new, o_run)

    none = torch.full_like(n_my, -1)
    at = lambda jh: torch.full_like(n_my, jh)                         # noqa: E731
    bA = torch.where(n_my > 0, at(0), none)
    bB = torch.where(n_my > 1, at(1), none)
    bC = none
    for jh in range(0, int(n_my.max()), 3):                           # the ring, guard for guard
        a0 = jh < n_my
        bC = torch.where(a0 & (jh + 2 < n_my), at(jh + 2), bC)
        reduce_half(jh, bA, a0)
        a1 = a0 & (jh + 1 < n_my)
        bA = torch.where(a1 & (jh + 3 < n_my), at(jh + 3), bA)
        reduce_half(jh + 1, bB, a1)
        a2 = a1 & (jh + 2 < n_my)
        bB = torch.where(a2 & (jh + 4 < n_my), at(jh + 4), bB)
        reduce_half(jh + 2, bB if name == "ring" else bC, a2)
    # the partials: every split below n_splits stores, the ones without a block (-inf, 0, 0)
    part_m = torch.full((B, H, ns), float("-inf"), dtype=f32, device=dev)
    part_l = torch.zeros(B, H, ns, dtype=f32, device=dev)
    part_o = torch.zeros(B, H, ns, HD, dtype=f32, device=dev)
    part_m[:, :, :S] = m_run.permute(0, 2, 1)
    part_l[:, :, :S] = _tree8(l_run, 3).permute(0, 2, 1)
    part_o[:, :, :S] = _tree8(o_run, 3).permute(0, 2, 1, 3)
    # attn_decode_combine_kernel: weights 2^(m_s - M), four groups take splits g, g + 4, ... in order, then meet
    M = part_m.amax(-1, keepdim=True)
    w = torch.where(part_m == ninf, torch.zeros_like(part_m), torch.exp2(part_m - M))
    L = torch.zeros(B, H, dtype=f32, device=dev)
    acc = torch.zeros(B, H, 4, HD, dtype=f32, device=dev)
    for sp in range(ns):
        L = L + part_l[:, :, sp] * w[:, :, sp]
        acc[:, :, sp % 4] = acc[:, :, sp % 4] + part_o[:, :, sp] * w[:, :, sp, None]
    tot = ((acc[:, :, 0] + acc[:, :, 1]) + acc[:, :, 2]) + acc[:, :, 3]
    o = torch.where(L[..., None] > 0, tot / L[..., None], torch.zeros_like(tot))
    return o.to(BF)[:, None], torch.stack([part_m, part_l], -1)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def differs(a, b):
    """(o, part_ml) pairs: any output bit or any partial statistic (by value; they are never NaN) differs."""
    return not (torch.equal(bits(a[0]), bits(b[0])) and torch.equal(a[1], b[1]))


# ------------------------------------------------------------------------------------------------ the largest admissible offset
BIG_TK = 2100


def largest_token_stride(Tk=BIG_TK):
    """The largest token stride in bytes (a multiple of 16) that evo_attn_decode_fp8 admits at Tk keys: Tk * d_st < 2^32 - 1."""
    return (0xffffffff - 1) // Tk // 16 * 16


# ------------------------------------------------------------------------------------------------ the write path's rows
def write_path_rows(B, T, H, device="cpu"):
    """bf16 rows for the quantising writers, [B, T, H, 128] each, such that dequant(quant_rule(row)) == row bit for bit (every element has
    at most 4 significant bits and a row's dynamic range fits e4m3 under the rule), and their levels:
      k   the base-16 digits of the token number + 1 (no all-zero row) in DIMSETS[1][:3], times 2^t(b, token) with t hashed in [-3, 3] (one
          per token: every head of a token carries the same power, so that a level is a property of (b, token)); with q = 8 G 16^i the
          level is (token + 1) 2^(t + 3), an integer in units of G.  Two tokens may tie; `expected` then returns the mean of their V rows.
      v   sign m 2^x with m in {0, 8 .. 15} and x in [0, 7], times 2^r with r hashed in [-10, 10] per (b, token, head).
      q   8 G 16^i on the digit dims; odd batch rows negated (the lowest level wins)."""
    dims = DIMSETS[1][:3]
    assert T < 16 ** 3
    j = torch.arange(T, dtype=torch.int64, device=device)
    tk = mix31(_key_index(B, T, 1, device), 81) % (2 * T_RANGE + 1) - T_RANGE                        # [B, T, 1]
    k = torch.zeros(B, T, H, HD, dtype=torch.float32, device=device)
    q = torch.zeros(B, 1, H, HD, dtype=torch.float32, device=device)
    sign = torch.tensor([1.0 if b % 2 == 0 else -1.0 for b in range(B)], device=device)[:, None, None]
    for i, d in enumerate(dims):
        k[..., d] = (((j + 1) // 16 ** i) % 16).float()[None, :, None] * pow2(tk)
        q[..., d] = sign * 8 * G * 16.0 ** i
    lev = (j + 1)[None, :] * (torch.ones_like(tk[:, :, 0]) << (tk[:, :, 0] + T_RANGE))
    lev = torch.where(sign[:, :, 0] > 0, lev, -lev)
    z = mix31(X._index(B, T, H, device), 82)
    m = z % 9                                                                                       # 0: a zero element
    mant = torch.where(m == 0, torch.zeros_like(m), m + 7).float()
    v = mant * pow2((z >> 4) % 8) * torch.where(m == 0, 0, (z >> 8) & 1).mul(-2.0).add(1.0)              # (no -0: a sum from +0 returns +0)
    v = v * pow2(mix31(_key_index(B, T, H, device), 83) % 21 - 10)[..., None]
    return q.to(BF), k.to(BF), v.to(BF), lev
