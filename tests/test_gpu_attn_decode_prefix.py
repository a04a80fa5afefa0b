"""GPU (-m gpu): decode attention behind SHARED stored prompts (evo_attn_decode_prefix_bf16: attn_decode_group_kernel for the store rows,
attn_decode_stream_kernel for the rows' own keys, one combine) and evo_rope_append_decode_at_bf16, on the EXACT key sets of
tests/attn_exact.py (record: DESIGN.md section 16).

A case is built on the CONCATENATION: row b's keys are [the store row's pre_len keys | its own keys 0 .. own_pos[b]], the multiplicities
are decode_mult(pre_len + own_pos, Tk).  The first batch row that names a store row lends its prefix (k, v, levels) to every other row
that names it; `expected` is general in levels and multiplicities, so the closed forms hold.  The store and the own caches are 0xFF
behind their lengths, part_o / part_ml are NaN before every launch, every launch is issued twice and must be bit-identical.  Both
kernels take a row's reference point from the very number they subtract (the streaming form): no row may hold an adjacent pattern,
plain or PRE.  Under U part_ml holds (0, the EXACT number of keys the split took): the interleaved block map of both partitions, and
(-inf, 0) for rows without a prefix.

The arena cases of the two new entries live here (tests/test_gpu_arena.py is not edited): `covers` registers them at import, as
tests/test_gpu_attn_prefix.py does."""
import math

import pytest
import torch

import attn_exact as X
from gpu_ref64 import causal_attention64
from test_gpu_arena import _run, covers, gen, poisoned, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
SLACK = 37                               # rows behind a store row's / a cache's capacity in use: 0xFF
H = 2
PRE_ROW = [0, 0, 1, -1, 0, 1, 1, 2, 2, 2, -1]          # B = 11: a ragged last tile for 4 and 8 rows per tile; three prompts and a
OWN_POS = [0, 1, 31, 32, 63, 64, 130, 0, 64, 130, 31]   # prefix-less row inside one tile
PRE_LENS = [(65, 2080, 1), (32, 64, 33)]
SPLITS = [(1, 1), (4, 4), (40, 8), None]


@pytest.fixture(scope="module")
def ops():
    from evo_amd.ops import HipOps
    return HipOps()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _plen(pre_row, pre_len):
    return [pre_len[r] if r >= 0 else 0 for r in pre_row]


def _leads(pre_row):
    return {r: pre_row.index(r) for r in set(pre_row) if r >= 0}


def _planted(pre_row, pre_len, own_pos, n_pre, n_own):
    """S: the block seams of the prefix partition (the same list for every row of a store row), both sides of the prefix / own seam, the
    block seams of the own partition."""
    out = []
    for r, own in zip(pre_row, own_pos):
        P = pre_len[r] if r >= 0 else 0
        ts = set(X.decode_seams(P, n_pre)) | {P - 2, P - 1} if P else set()
        ts |= {P, P + 1} | {P + t for t in X.decode_seams(own + 1, n_own)}
        out.append(sorted(t for t in ts if 0 <= t <= P + own))
    return out


def _build(design, pre_row, pre_len, own_pos, dims, n_pre, n_own, alt=False):
    B, plen = len(pre_row), _plen(pre_row, pre_len)
    total = [p + o for p, o in zip(plen, own_pos)]
    Tk = max(total) + 1
    planted = _planted(pre_row, pre_len, own_pos, n_pre, n_own) if design == "S" else None
    c = X.build_case(design, B, H, 1, 0, Tk, dims, DEV, planted=planted, alt=alt, mult=X.decode_mult(total, Tk, DEV))
    for r, lead in _leads(pre_row).items():                              # the lead row's prefix IS the store row
        P = pre_len[r]
        for b in range(B):
            if pre_row[b] == r and b != lead:
                c["k"][b, :P], c["v"][b, :P], c["lev"][b, :P] = c["k"][lead, :P], c["v"][lead, :P], c["lev"][lead, :P]
    return c


def _place(c, pre_row, pre_len, own_pos, P_cap, cap, R):
    """-> store [R + 1, P_cap, 2, H, 128] and own caches [B + 1, cap, 2, H, 128], 0xFF behind every length."""
    B, plen = len(pre_row), _plen(pre_row, pre_len)
    store = poisoned((R + 1, P_cap, 2, H, 128), BF)
    for r, lead in _leads(pre_row).items():
        store[r, :pre_len[r], 0], store[r, :pre_len[r], 1] = c["k"][lead, :pre_len[r]], c["v"][lead, :pre_len[r]]
    kv = poisoned((B + 1, cap, 2, H, 128), BF)
    for b in range(B):
        n, P = own_pos[b] + 1, plen[b]
        kv[b, :n, 0], kv[b, :n, 1] = c["k"][b, P:P + n], c["v"][b, P:P + n]
    return store, kv


def _i64(x):
    return torch.tensor(list(x), dtype=torch.int64, device=DEV)


def _call(ops, q, kv, store, R, pre_row, pre_len, own_pos, n_pre, n_own, pre):
    """The C entry as HipOps.attention_decode_prefix calls it, with caller-owned NaN-filled part_o / part_ml; two launches, all three
    outputs bit-identical.  -> (o [B, 1, H, 128], part_ml [B, H, n_pre + n_own, 2])"""
    from evo_amd.ops import _check, _stream
    B = q.shape[0]
    k, v, ks, vs = kv[:B, :, 0], kv[:B, :, 1], store[:R, :, 0], store[:R, :, 1]
    row, ln, own = _i64(pre_row), _i64(pre_len), _i64(own_pos)
    outs = []
    for _ in range(2):
        o = poisoned((B, 1, H, 128), BF)
        part_o = poisoned((B, H, n_pre + n_own, 128), torch.float32)
        part_ml = poisoned((B, H, n_pre + n_own, 2), torch.float32)
        _check(ops.lib.evo_attn_decode_prefix_bf16(
            q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), B, H, k.shape[1], q.stride(0), q.stride(2),
            k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1), v.stride(2), own.data_ptr(),
            ks.data_ptr(), vs.data_ptr(), R, ks.shape[1], ks.stride(0), ks.stride(1), ks.stride(2), vs.stride(0), vs.stride(1), vs.stride(2),
            row.data_ptr(), ln.data_ptr(), part_o.data_ptr(), part_ml.data_ptr(), n_pre, n_own, 0.0 if pre else 1.0 / math.sqrt(128),
            _stream()), "evo_attn_decode_prefix_bf16")
        outs.append((o, part_o, part_ml))
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(_bits(a), _bits(b)), "two launches differ"
    return outs[0][0], outs[0][2]


def _judge(got, c, what):
    ref, single = X.expected(c["lev"], c["v"], c["mult"])
    ver = X.judge(got, ref, single, None)                                # the stream form: no adjacent patterns, plain or PRE
    print(f"[decode prefix] {what}: {ver}")
    assert ver.ok, f"{what}: {ver}; first bad rows (b, query) {ver.bad.nonzero()[:8].tolist()}"


def _assert_counts(part_ml, pre_row, pre_len, own_pos, n_pre, n_own, what):
    B = len(pre_row)
    want = torch.empty(B, H, n_pre + n_own, 2, dtype=torch.float32)
    for b in range(B):
        pc = X.stream_split_counts(pre_len[pre_row[b]], n_pre) if pre_row[b] >= 0 else [0] * n_pre
        cnt = torch.tensor(pc + X.stream_split_counts(own_pos[b] + 1, n_own), dtype=torch.float32)
        want[b, :, :, 0] = torch.where(cnt > 0, 0.0, float("-inf"))[None, :]
        want[b, :, :, 1] = cnt[None, :]
    got = part_ml.cpu()
    bad = (got != want).any(-1)
    assert not bool(bad.any()), f"{what}: per-split (m, l) differ from the documented partitions at (b, h, split) {bad.nonzero()[:8].tolist()}: " \
                                f"got {got[bad][:4].tolist()} want {want[bad][:4].tolist()}"


def _dims(n):
    return (X.DIMS2 + X.DIMS3)[n % 5]


@pytest.mark.parametrize("sp", SPLITS, ids=["splits" + ("-default" if s is None else f"{s[0]}+{s[1]}") for s in SPLITS])
@pytest.mark.parametrize("pl", range(len(PRE_LENS)), ids=["len" + "-".join(map(str, p)) for p in PRE_LENS])
def test_decode_prefix_on_exact_key_sets(ops, pl, sp):
    pre_len = PRE_LENS[pl]
    R, P_cap, cap = 3, max(pre_len) + SLACK, max(OWN_POS) + 1 + SLACK
    n_pre, n_own = (ops._decode_splits(P_cap), ops._decode_splits(cap)) if sp is None else sp
    for i, design in enumerate(X.DESIGNS):
        c = _build(design, PRE_ROW, pre_len, OWN_POS, _dims(i + n_pre + pl), n_pre, n_own)
        store, kv = _place(c, PRE_ROW, pre_len, OWN_POS, P_cap, cap, R)
        for pre in (False, True):
            what = f"{design} {'PRE' if pre else 'plain'} pre_len {pre_len} splits {n_pre}+{n_own} dims {c['dims']}"
            o, part_ml = _call(ops, c["q"], kv, store, R, PRE_ROW, pre_len, OWN_POS, n_pre, n_own, pre)
            _judge(o, c, what)
            if design == "U":
                _assert_counts(part_ml, PRE_ROW, pre_len, OWN_POS, n_pre, n_own, what)


def test_decode_prefix_long_store_row(ops):
    """A store row of 70,000 keys in a store of capacity 131,072 (the 32-bit key offsets at H = 2: 268 MB per row), two rows that share
    it and one without; U on V_alt: one lost key flips an output between 0 and 1 / n at any length."""
    pre_row, pre_len, own_pos = [0, -1, 0], (70000,), [130, 64, 0]
    R, P_cap, cap = 1, 131072, 131 + SLACK
    n_pre, n_own = ops._decode_splits(P_cap), ops._decode_splits(cap)
    c = _build("U", pre_row, pre_len, own_pos, X.DIMS3[0], n_pre, n_own, alt=True)
    store, kv = _place(c, pre_row, pre_len, own_pos, P_cap, cap, R)
    for pre in (False, True):
        what = f"long U {'PRE' if pre else 'plain'} splits {n_pre}+{n_own}"
        o, part_ml = _call(ops, c["q"], kv, store, R, pre_row, pre_len, own_pos, n_pre, n_own, pre)
        _judge(o, c, what)
        _assert_counts(part_ml, pre_row, pre_len, own_pos, n_pre, n_own, what)


@pytest.mark.parametrize("pre", [False, True])
def test_decode_prefix_randn_vs_fp64(ops, pre):
    """N(0, 1.5^2) queries, N(0, 1) keys / values against fp64 attention on the concatenation, through the binding and its default split
    counts, under PARITY row 22c's bound: rel-L2 <= 4e-3 per batch row, |err| <= 2^-8 |ref| + 2e-2."""
    pre_len = PRE_LENS[0]
    B, R, P_cap, cap = len(PRE_ROW), 3, max(pre_len) + SLACK, max(OWN_POS) + 1 + SLACK
    g = gen(77 + int(pre))
    store, kv = poisoned((R + 1, P_cap, 2, H, 128), BF), poisoned((B + 1, cap, 2, H, 128), BF)
    for r, n in enumerate(pre_len):
        store[r, :n] = rnd((n, 2, H, 128), g)
    for b, p in enumerate(OWN_POS):
        kv[b, :p + 1] = rnd((p + 1, 2, H, 128), g)
    q = rnd((B, 1, H, 128), g, 1.5)
    cs = ops.attn_q_scale(128)
    qq = (q.float() * cs).to(BF) if pre else q
    o = ops.attention_decode_prefix(qq, kv[:B, :, 0], kv[:B, :, 1], _i64(OWN_POS), store[:R, :, 0], store[:R, :, 1], _i64(PRE_ROW), _i64(pre_len),
                                    prescaled=pre)
    torch.cuda.synchronize()
    got = o.double()
    assert torch.isfinite(got).all()
    worst_rl2, worst_excess = 0.0, -1.0
    for b, (r, p) in enumerate(zip(PRE_ROW, OWN_POS)):
        P = pre_len[r] if r >= 0 else 0
        kvc = torch.cat([store[r, :P], kv[b, :p + 1]], 0) if P else kv[b, :p + 1]
        q_ref = qq[b].double() / cs if pre else qq[b]
        ref = causal_attention64(q_ref, kvc[:, 0], kvc[:, 1], _i64([P + p]))
        err = got[b] - ref
        worst_rl2 = max(worst_rl2, (err.norm() / ref.norm()).item())
        worst_excess = max(worst_excess, (err.abs() - (ref.abs() * 2 ** -8 + 2e-2)).max().item())
    print(f"[decode prefix] randn {'PRE' if pre else 'plain'}: worst row rel-L2 {worst_rl2:.3e}, worst |err| - (2^-8 |ref| + 2e-2) = {worst_excess:+.3e}")
    assert worst_rl2 <= 4e-3 and worst_excess <= 0.0


# ================================================================================================ rotary + append at a given row
def _rope_inputs(B, cap, seed):
    g = gen(seed)
    inv = (1.0 / (10000.0 ** (torch.arange(0, 128, 2, dtype=torch.float32, device=DEV) / 128))).contiguous()
    return rnd((B, 1, 3, H, 128), g), inv


@pytest.mark.parametrize("q_scale", [1.0, None])
def test_rope_append_at_is_the_existing_entry_when_widx_is_pos(ops, q_scale):
    positions, cap = [0, 39, 17, 5, 38], 40
    B = len(positions)
    qkv, inv = _rope_inputs(B, cap, 3)
    qs = ops.attn_q_scale(128) if q_scale is None else q_scale
    pos = _i64(positions)
    a, b = qkv.clone(), qkv.clone()
    kv_a, kv_b = poisoned((B + 1, cap, 2, H, 128), BF), poisoned((B + 1, cap, 2, H, 128), BF)
    ops.rope_append_decode(a, kv_a[:B], pos, inv, 16.0, q_scale=qs)
    ops.rope_append_decode(b, kv_b[:B], pos, inv, 16.0, q_scale=qs, widx=pos.clone())
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(kv_a), _bits(kv_b))


@pytest.mark.parametrize("q_scale", [1.0, None])
def test_rope_append_at_rotates_by_pos_and_writes_row_widx(ops, q_scale):
    positions, rows, cap = [100, 39, 8191, 5, 70000], [0, 39, 17, 5, 38], 40
    B = len(positions)
    qkv, inv = _rope_inputs(B, cap, 4)
    qs = ops.attn_q_scale(128) if q_scale is None else q_scale
    pos, widx = _i64(positions), _i64(rows)
    a, b = qkv.clone(), qkv.clone()
    kv_a, kv_b = poisoned((B + 1, 70001, 2, H, 128), BF), poisoned((B + 1, cap, 2, H, 128), BF)
    ops.rope_append_decode(a, kv_a[:B], pos, inv, 16.0, q_scale=qs)      # the existing entry: q and k of `pos`
    ops.rope_append_decode(b, kv_b[:B], pos, inv, 16.0, q_scale=qs, widx=widx)
    torch.cuda.synchronize()
    assert torch.equal(_bits(a), _bits(b))
    ar = torch.arange(B, device=DEV)
    assert torch.equal(_bits(kv_b[ar, widx]), _bits(b[:, 0, 1:3]))        # (k rotated, v) at row widx
    assert torch.equal(_bits(kv_b[ar, widx]), _bits(kv_a[ar, pos]))
    written = torch.zeros(B + 1, cap, dtype=torch.bool, device=DEV)
    written[ar, widx] = True
    still = (kv_b.contiguous().view(B + 1, cap, -1).view(torch.uint8) == 0xFF).all(-1)
    assert torch.equal(still, ~written)                                  # ... and nothing else changed


# ================================================================================================ arena
@covers("evo_attn_decode_prefix_bf16")
@pytest.mark.parametrize("pre", [False, True])
def test_arena_decode_prefix(pre):
    """The store and the own caches as strided views of [R, cap, 2, H, 128] buffers placed at 16-byte alignment, 0xFF behind their
    lengths; the partial buffers and the output are allocated by the binding (carved from the poisoned arena)."""
    from evo_amd.ops import default_ops
    ops, g = default_ops(), gen(21)
    pre_len = PRE_LENS[0]
    B, R, P_cap, cap = len(PRE_ROW), 3, max(pre_len) + SLACK, max(OWN_POS) + 1 + SLACK
    store, kv = poisoned((R, P_cap, 2, H, 128), BF), poisoned((B, cap, 2, H, 128), BF)
    for r, n in enumerate(pre_len):
        store[r, :n] = rnd((n, 2, H, 128), g)
    for b, p in enumerate(OWN_POS):
        kv[b, :p + 1] = rnd((p + 1, 2, H, 128), g)
    inp = {"q": rnd((B, 1, H, 128), g, ops.attn_q_scale(128) if pre else 1.0), "kv": kv, "store": store, "own": _i64(OWN_POS),
           "row": _i64(PRE_ROW), "ln": _i64(pre_len)}
    _run(lambda q, kv, store, own, row, ln: ops.attention_decode_prefix(q, kv[:, :, 0], kv[:, :, 1], own, store[:, :, 0], store[:, :, 1], row, ln,
                                                                        prescaled=pre),
         inp, expect=["evo_attn_decode_prefix_bf16"], align={"own": 8, "row": 8, "ln": 8})


@covers("evo_rope_append_decode_at_bf16")
def test_arena_rope_append_at():
    from evo_amd.ops import default_ops
    ops = default_ops()
    positions, rows, cap = [100, 39, 8191, 5, 70000], [0, 39, 17, 5, 38], 40
    B = len(positions)
    qkv, inv = _rope_inputs(B, cap, 5)
    inp = {"qkv": qkv, "kv": poisoned((B + 1, cap, 2, H, 128), BF), "pos": _i64(positions), "widx": _i64(rows), "inv": inv}
    _run(lambda qkv, kv, pos, widx, inv: ops.rope_append_decode(qkv, kv[:B], pos, inv, 16.0, widx=widx), inp, inout=["qkv", "kv"],
         expect=["evo_rope_append_decode_at_bf16"], align={"pos": 8, "widx": 8})
