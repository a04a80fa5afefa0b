"""GPU (-m gpu): the attention kernels on EXACT key sets (tests/attn_exact.py; PARITY rows 12a and 22g).

Every softmax weight of these inputs is exactly 1 or 0, so a row's output says which keys it saw: D / D' / S rows must return one V row
bit for bit, U rows bf16(count / n) (the adjacent pattern only within 2^-21 |ref| of a rounding boundary, at most 0.1 % of a case).  No
tensor-wide term.  Every launch is issued twice; the pair must be bit-identical.  What is checked where:
  prefill   HipOps.attention: the 64-rows-per-wave kernel (mask_from / mask_nxt / lim_rel / q_pad, both block maps), the 8-wave kernel
            (ops.attn_w64 = False), the 128-row kernel; q / k / v as thirds of a packed qkv or k / v as views of a [B, cap, 2, H, 128] cache
            whose rows behind Tk are 0xFF; keys inside Tk that nobody sees are 2^100
  prefix    HipOps.attention_prefix: the SEG seam; V_hist counts and planted keys run across it; the plane of a longer prefix
  decode    evo_attn_decode_bf16 through the C entry with caller-owned NaN-filled part_o / part_ml, one position per row.  Under U
            part_ml holds (0, the EXACT number of keys the split took) -- equal to the partition each kernel documents (streaming: blocks
            s, s + n_splits, ...; attn_fwd_kernel<true>: ceil(n_tiles / n_splits) consecutive tiles; empty splits (-inf, 0)), which also
            proves which kernel ran.

Plain form, winner's weight.  attn_fwd_w64_kernel and attn_decode_stream_kernel take a row's reference point from the very fp32 number
they subtract, so the winner's exponent is exactly 0, P = l = 1 and the output is the V row's pattern.  attn_fwd_kernel<.> and
attn_fwd_pipe_kernel form m = fl(tmax c) and then e = fma(s, c, -m) = s c - fl(s c) =: r, |r| <= ulp(s c) / 2: P = 2^r, l = fl(2^r)
(unrounded), and the output is bf16(v bf16(P) / l).  The smallest relative half-spacing of bf16 is 2^-9 (at either side of a power of
two).  While |s c| < 2^16, ulp(s c) <= 2^-8 and |r| ln 2 <= 2^-9 ln 2 = 1.35e-3 < 2^-9: bf16(P) = 1 and v / l rounds back to v -- bit exact.
From |s c| >= 2^16 on (D rows whose last key is j >= 251: s = 2,048 j) |r| reaches 2^-8, bf16(P) may differ from 1 and |bf16(P) / l - 1|
<= 1.02 * 2^-9 can cross one rounding boundary but not two: the result is v or the ADJACENT pattern.  Those rows -- plain form, these three
kernels, |winner's s c| >= 2^16 -- may hold the adjacent pattern (`_adjacent_rows`; V_id rows differ by more than one pattern in >= 100
of 128 dims, so a wrong key still fails; the count is printed); every other row, and every
PRE row (c = 1: r = 0), is bit for bit.
"""
import math

import pytest
import torch

import attn_exact as X

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
SLACK = 37                               # cache rows behind Tk / the prefix: 0xFF


@pytest.fixture(scope="module")
def ops():
    from evo_amd.ops import HipOps
    return HipOps()


def _poisoned(shape, dtype=BF):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(-1).view(torch.uint8).fill_(0xFF)
    return t


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _twice(fn):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), _bits(b)), "two launches differ"
    return a


def _adjacent_rows(kind, pre, c):
    """See the module docstring: rows that may hold the adjacent pattern."""
    if pre or kind in ("w64", "stream"):
        return None
    low = torch.iinfo(torch.int64).min
    top = torch.where(c["mult"] > 0, c["lev"][:, None, :], torch.full_like(c["mult"], low)).max(-1).values
    return top.abs().double() * X.G * X.C_LOG2 >= 2.0 ** 16


def _judge(got, c, kind, pre, what):
    ref, single = X.expected(c["lev"], c["v"], c["mult"])
    ver = X.judge(got, ref, single, _adjacent_rows(kind, pre, c))
    print(f"[attn exact] {what}: {ver}")
    assert ver.ok, f"{what}: {ver}; first bad rows (b, query) {ver.bad.nonzero()[:8].tolist()}"
    return ver


def _dims(n):
    return (X.DIMS2 + X.DIMS3)[n % 5]


# ================================================================================================ prefill
def _prefill(ops, c, q_pos0, pre):
    """q / k / v as thirds of a packed qkv where the shapes allow it (q_pos0 = 0, Tk = Tq), else k / v as views of a [B, cap, 2, H, 128]
    cache whose rows behind Tk are 0xFF."""
    q, k, v = c["q"], c["k"], c["v"]
    B, Tq, H, _ = q.shape
    Tk = k.shape[1]
    if q_pos0 == 0 and Tk == Tq:
        qkv = torch.stack([q, k, v], 2)
        qq, kk, vv = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]
    else:
        kv = _poisoned((B, Tk + SLACK, 2, H, 128))
        kv[:, :Tk, 0], kv[:, :Tk, 1] = k, v
        qq, kk, vv = q.contiguous(), kv[:, :Tk, 0], kv[:, :Tk, 1]
    return _twice(lambda: ops.attention(qq, kk, vv, q_pos0, prescaled=pre))


def _prefill_cases(ops, kind, shape, B, H, n):
    Tq, q_pos0, dTk = shape
    Tk = q_pos0 + Tq + dTk
    for i, design in enumerate(X.DESIGNS):
        c = X.build_case(design, B, H, Tq, q_pos0, Tk, _dims(n + i), DEV)
        for pre in (False, True):
            got = _prefill(ops, c, q_pos0, pre)
            _judge(got, c, kind, pre, f"{kind} {design} {'PRE' if pre else 'plain'} B {B} H {H} Tq {Tq} q_pos0 {q_pos0} Tk {Tk} dims {c['dims']}")


_W64 = [(s, 3, 2) for s in X.W64_SHAPES] + [(s, 1, 2) for s in (X.W64_SHAPES[3], X.W64_SHAPES[7])] \
    + [(s, 1, 8) for s in (X.W64_SHAPES[0], X.W64_SHAPES[4], X.W64_SHAPES[6], X.W64_SHAPES[9])]


@pytest.mark.parametrize("n", range(len(_W64)), ids=[f"Tq{s[0]}-p{s[1]}-d{s[2]}-B{b}H{h}" for s, b, h in _W64])
def test_w64_prefill_on_exact_key_sets(ops, n):
    """attn_fwd_w64_kernel<PRE>: query blocks aligned to the END of the range (q_pad), the first masked tile (mask_from), the ragged last
    tile, canaries inside Tk; 8 (batch, head) pairs take the XCD block map."""
    shape, B, H = _W64[n]
    assert shape[0] > 128 and ops.attn_w64
    _prefill_cases(ops, "w64", shape, B, H, n)


@pytest.mark.parametrize("n", range(len(X.PIPE_SHAPES)), ids=[f"Tq{s[0]}-p{s[1]}" for s in X.PIPE_SHAPES])
def test_pipe_prefill_on_exact_key_sets(ops, n):
    """attn_fwd_pipe_kernel (the 8-wave kernel: no V^T workspace)."""
    ops.attn_w64 = False
    try:
        _prefill_cases(ops, "pipe", X.PIPE_SHAPES[n], 3, 2, n + 1)
    finally:
        ops.attn_w64 = True


@pytest.mark.parametrize("n", range(len(X.QB128_SHAPES)), ids=[f"Tq{s[0]}-p{s[1]}" for s in X.QB128_SHAPES])
def test_qb128_prefill_on_exact_key_sets(ops, n):
    """attn_fwd_kernel<false>: query ranges of at most one 128-row block."""
    assert X.QB128_SHAPES[n][0] <= 128
    _prefill_cases(ops, "qb128", X.QB128_SHAPES[n], 3, 2, n + 2)


# ================================================================================================ shared prefix
@pytest.mark.parametrize("P,Tq", X.PREFIX_SHAPES)
def test_prefix_attention_on_exact_key_sets(ops, P, Tq):
    """evo_attn_fwd_prefix_bf16 (SEG): every batch row its own suffix data and planted keys (P - 1 and P among them), V_hist counts run
    across the seam; the prefix is a view of a [1, P + 37, 2, H, 128] cache; the V^T plane of a LONGER prefix serves this one."""
    B, H = 3, 2
    for i, design in enumerate(X.DESIGNS):
        c = X.build_case(design, B, H, Tq, P, P + Tq, _dims(P // 64 + Tq + i), DEV, shared_prefix=P)
        kvp = _poisoned((1, P + SLACK, 2, H, 128))
        kvp[0, :P, 0], kvp[0, :P, 1] = c["k"][0, :P], c["v"][0, :P]
        qkv = torch.stack([c["q"], c["k"][:, P:], c["v"][:, P:]], 2)
        kv2 = _poisoned((1, P + 128 + SLACK, 2, H, 128))
        kv2[:, :P] = kvp[:, :P]
        kv2[:, P:P + 128] = X.CANARY                                    # the longer prefix's own keys: finite, visible to nobody here
        plane = ops.attention_prefix_vt(kv2[0, :P + 128, 1])
        for pre in (False, True):
            what = f"prefix {design} {'PRE' if pre else 'plain'} P {P} Tq {Tq} dims {c['dims']}"
            got = _twice(lambda: ops.attention_prefix(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], kvp[0, :P, 0], kvp[0, :P, 1], prescaled=pre))
            _judge(got, c, "w64", pre, what)
            got2 = _twice(lambda: ops.attention_prefix(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], kv2[0, :P, 0], None, vt_pre=plane, prescaled=pre))
            assert torch.equal(_bits(got2), _bits(got)), what + ": the longer prefix's plane"


# ================================================================================================ decode
def _decode(ops, q, k, v, positions, n_splits, pre):
    """The C entry as HipOps.attention_decode calls it, with caller-owned part_o / part_ml pre-filled with NaN; two launches, all three
    outputs bit-identical.  -> (o [B, 1, H, 128], part_ml [B, H, n_splits, 2])"""
    from evo_amd.ops import _check, _stream
    B, _, H, hd = q.shape
    Tk = k.shape[1]
    pos = torch.tensor(positions, dtype=torch.int64, device=DEV)
    outs = []
    for _ in range(2):
        o = _poisoned((B, 1, H, hd))
        part_o = _poisoned((B, H, n_splits, hd), torch.float32)
        part_ml = _poisoned((B, H, n_splits, 2), torch.float32)
        _check(ops.lib.evo_attn_decode_bf16(
            q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), B, H, Tk, q.stride(0), q.stride(2),
            k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1), v.stride(2), pos.data_ptr(),
            part_o.data_ptr(), part_ml.data_ptr(), n_splits, 0.0 if pre else 1.0 / math.sqrt(hd), _stream()), "evo_attn_decode_bf16")
        outs.append((o, part_o, part_ml))
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(_bits(a), _bits(b)), "two launches differ"
    return outs[0][0], outs[0][2]


def _default_splits(Tk):
    return min(((Tk + 63) // 64 + 3) // 4 * 4, 32)                      # HipOps.attention_decode


def _assert_split_counts(part_ml, positions, n_splits, counts_of, what):
    """U: every exponent is 0 and every weight 1, so a split's (m, l) is (0, the number of keys it took) or (-inf, 0) when it took none."""
    B, H = part_ml.shape[:2]
    want = torch.empty(B, H, n_splits, 2, dtype=torch.float32)
    for b, p in enumerate(positions):
        cnt = torch.tensor(counts_of(p + 1, n_splits), dtype=torch.float32)
        want[b, :, :, 0] = torch.where(cnt > 0, 0.0, float("-inf"))[None, :]
        want[b, :, :, 1] = cnt[None, :]
    got = part_ml.cpu()
    bad = (got != want).any(-1)
    assert not bool(bad.any()), f"{what}: per-split (m, l) differ from the documented partition at (b, h, split) {bad.nonzero()[:8].tolist()}: " \
                                f"got {got[bad][:4].tolist()} want {want[bad][:4].tolist()}"


def _cache_views(c, positions, cap):
    """[B + 1, cap, 2, H, 128], 0xFF everywhere except each row's keys 0 .. position."""
    B, H = len(positions), c["k"].shape[2]
    kv = _poisoned((B + 1, cap, 2, H, 128))
    for b, p in enumerate(positions):
        kv[b, :p + 1, 0], kv[b, :p + 1, 1] = c["k"][b, :p + 1], c["v"][b, :p + 1]
    return kv[:B, :, 0], kv[:B, :, 1]


@pytest.mark.parametrize("ns", X.DECODE_SPLITS, ids=[f"splits{ns}" for ns in X.DECODE_SPLITS])
def test_decode_stream_on_exact_key_sets(ops, ns):
    """attn_decode_stream_kernel + attn_decode_combine_kernel: positions around every 32-key half and 64-key block, two long rows, mixed
    in one batch; the interleaved block-to-split map is read back from part_ml."""
    positions, H = X.DECODE_POSITIONS, 2
    cap = max(positions) + 1 + SLACK
    n_splits = _default_splits(cap) if ns is None else ns
    assert cap * 2 * H * 128 * 2 < 0xffffffff                          # the streaming kernel's condition
    for i, design in enumerate(X.DESIGNS):
        c = X.build_decode(design, positions, H, _dims(i + n_splits), n_splits, DEV)
        k, v = _cache_views(c, positions, cap)
        for pre in (False, True):
            what = f"decode stream {design} {'PRE' if pre else 'plain'} n_splits {n_splits} dims {c['dims']}"
            o, part_ml = _decode(ops, c["q"], k, v, positions, n_splits, pre)
            _judge(o, c, "stream", pre, what)
            if design == "U":
                _assert_split_counts(part_ml, positions, n_splits, X.stream_split_counts, what)


@pytest.mark.parametrize("design", ["U", "D"])
def test_decode_stream_long_cache(ops, design):
    """cap = 131,072, H = 2, positions 0 / 70,000 / 131,071: U on V_alt (one lost key flips an output between 0 and 1 / n at any length; a
    lost run of 256 ALIGNED keys cancels -- V_hist at the shorter lengths sees that), D with the three-dim keys."""
    positions, H, cap = X.LONG_POSITIONS, 2, X.LONG_CAP
    n_splits = _default_splits(cap)
    c = X.build_decode(design, positions, H, X.DIMS3[0], n_splits, DEV, alt=True, Tk=cap)
    k, v = _cache_views(c, positions, cap)
    for pre in (False, True):
        what = f"decode stream long {design} {'PRE' if pre else 'plain'} n_splits {n_splits}"
        o, part_ml = _decode(ops, c["q"], k, v, positions, n_splits, pre)
        _judge(o, c, "stream", pre, what)
        if design == "U":
            _assert_split_counts(part_ml, positions, n_splits, X.stream_split_counts, what)


# ================================================================================================ decode beyond 4 GiB: attn_fwd_kernel<true>
MFMA_TK, MFMA_ST = 2100, 1 << 20         # keys; token stride in elements (2 MiB)
MFMA_PAIRS = [(0, 2099), (2050, 63), (64, 2099)]


@pytest.fixture(scope="module")
def big():
    """One allocation of 4.4 GiB of bf16, never filled: tokens 2 MiB apart, [B = 2, 2, H = 2, 128] inside a token's slot."""
    return torch.empty((MFMA_TK - 1) * MFMA_ST + 2 * 2 * 2 * 128, dtype=BF, device=DEV)


def _big_views(big, c, positions):
    B, H = 2, 2
    k = big.as_strided((B, MFMA_TK, H, 128), (2 * H * 128, MFMA_ST, 128, 1), 0)
    v = big.as_strided((B, MFMA_TK, H, 128), (2 * H * 128, MFMA_ST, 128, 1), H * 128)
    for b, p in enumerate(positions):
        k[b, :p + 1], v[b, :p + 1] = c["k"][b, :p + 1], c["v"][b, :p + 1]
    # the dispatch condition of evo_attn_decode_bf16: 32-bit key offsets do not reach -> the MFMA split kernel
    assert MFMA_TK * k.stride(1) * 2 >= 0xffffffff and MFMA_TK * v.stride(1) * 2 >= 0xffffffff
    assert (max(positions) * MFMA_ST) * 2 > 1 << 32                     # keys lie BEYOND the 4 GiB offset
    return k, v


@pytest.mark.parametrize("ns", X.MFMA_SPLITS)
def test_decode_mfma_split_kernel_beyond_4gib(ops, big, ns):
    """attn_fwd_kernel<true>, reached as the product would reach it: k / v views with Tk * k_st * 2 >= 2^32 - 1 (token stride 2 MiB, Tk =
    2,100), positions {0, 63, 64, 2050, 2099} in pairs, n_splits {1, 3, 7, 64} (64: more splits than tiles).  Under U part_ml equals
    the CONTIGUOUS partition -- with 3 and 7 splits it differs from the streaming kernel's interleaved one.

    Address arithmetic, read before the first run (csrc/attn.hip, ATTN_ISSUE_LOADS in DECODE mode): kp / vp = base + bat * k_sb + head * k_sh
    are 64-bit pointers; a tile's base kb_ = kp + k0_ * a.k_st has k0_ int64, so the 4.4e9-byte offset of tile 32 is formed in 64 bits.
    The per-lane part (uint32_t)kk * kst_b + kc * 16 has kk <= rel_max_ <= 63 and kst_b = (uint32_t)(k_st * 2) = 2^21: at most 63 * 2^21 +
    240 < 2^27, no wrap; kst_b itself needs k_st * 2 < 2^32.  rel_max_ = min(63, Tk_ - 1 - k0_) with Tk_ = dyn_pos[bat] + 1 clamps every
    row of a ragged tile to the row's own last key, tiles run over [tile_begin, min(tile_begin + per, n_tiles)) with n_tiles = pos / 64 + 1:
    no load behind a row's position.  q: every lane reads row 0 (q_st = 0, qrow_c = 0).  part_o / part_ml: slot = (bat * H + head) *
    n_splits + blockIdx.x < B * H * n_splits.  A split past the last tile keeps (m, l, O) = (-inf, 0, 0) and stores that."""
    H = 2
    for positions in MFMA_PAIRS:
        for i, design in enumerate(("U", "D", "S")):
            c = X.build_decode(design, list(positions), H, _dims(i + ns), ns, DEV)
            k, v = _big_views(big, c, positions)
            for pre in (False, True):
                what = f"decode MFMA split {design} {'PRE' if pre else 'plain'} positions {positions} n_splits {ns} dims {c['dims']}"
                o, part_ml = _decode(ops, c["q"], k, v, list(positions), ns, pre)
                _judge(o, c, "mfma_split", pre, what)
                if design == "U":
                    _assert_split_counts(part_ml, positions, ns, X.mfma_split_counts, what)


@pytest.mark.parametrize("pre", [False, True])
def test_decode_mfma_split_kernel_randn_vs_fp64(ops, big, pre):
    """N(0, 1.5^2) queries and N(0, 1) keys / values against the fp64 oracle under row 22c's bound (rel-L2 <= 4e-3 per case and per batch
    row, |err| <= 2^-8 |ref| + 2e-2)."""
    from oracle import stripedhyena_ref as R
    positions, H, ns = [2099, 64], 2, 7
    g = torch.Generator(device=DEV).manual_seed(31)
    c = {"k": torch.randn(2, MFMA_TK, H, 128, device=DEV, generator=g).to(BF), "v": torch.randn(2, MFMA_TK, H, 128, device=DEV, generator=g).to(BF)}
    q = (torch.randn(2, 1, H, 128, device=DEV, generator=g) * 1.5).to(BF)
    cs = ops.attn_q_scale(128)
    qq = (q.float() * cs).to(BF) if pre else q
    q_ref = (qq.double() / cs if pre else qq).cpu()
    k, v = _big_views(big, c, positions)
    o, _ = _decode(ops, qq, k, v, positions, ns, pre)
    ref = torch.cat([R.op_attention(q_ref[b:b + 1], c["k"][b:b + 1, :p + 1].cpu(), c["v"][b:b + 1, :p + 1].cpu(), p) for b, p in enumerate(positions)], 0)
    got = o.double().cpu()
    rl2 = max(((got - ref).norm() / ref.norm()).item(), ((got - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)).max().item())
    excess = ((got - ref).abs() - (ref.abs() * 2 ** -8 + 2e-2)).max().item()
    print(f"[attn exact] decode MFMA split randn {'PRE' if pre else 'plain'}: rel-L2 {rl2:.3e}, worst |err| - (2^-8 |ref| + 2e-2) = {excess:+.3e}")
    assert torch.isfinite(got).all() and rl2 <= 4e-3 and excess <= 0.0
