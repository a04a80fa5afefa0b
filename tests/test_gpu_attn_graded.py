"""GPU (-m gpu): the attention kernels on exact GRADED softmax weights (design G of tests/attn_exact.py; PARITY row 12b).

The exact-key-set tests (tests/test_gpu_attn_exact.py and its siblings) make every softmax weight 1 or 0: they pin WHICH keys a row sees
and cannot see how keys are weighted -- every rescale factor there is 0 or 1.  Here every weight is an exact power of two: a score is
an integer exponent mu_i e_j, V = V_hist makes every output dim its own accumulator of sum 2^(mu e_j), and under the builder's condition
every weight, every partial sum of l and of any output dim is exact in fp32 in any order under any power-of-two reference.  Only 1 / l
and the last multiply round, so a FLAT row must equal bf16(the fp64 softmax) (the adjacent pattern only within 2^-21 |ref| of a rounding
boundary, at most 0.1 % of a case), and a STAIR row -- levels 31 / 32 / 33 and 63 / 64 / 65 units apart straddle the kernels' deferred-
maximum thresholds W_THR and W_THRP, a first tile at -65, drops of 40 and 70 -- within (64-key blocks visited + non-empty splits + 2)
fp32 roundings of 2^-24 on the same boundary rule.  No tensor-wide term; every element is judged.  Every launch is issued twice on
poisoned outputs; the pair must be bit-identical.

Two forms from one data set: PRE (softmax_scale <= 0: the score IS the exponent) and the plain form at softmax_scale = G_LN2, where the
entries' own scale_log2 = softmax_scale * log2(e) is 1.0f exactly (fma(s, c, -m), the running maximum, W_THR = 32 are the plain code
paths).  That scale is no parameter of HipOps, so the C entries are called directly, the way HipOps calls them.

Everything rests on v_exp_f32 returning the exact power of two for an integer argument (the ISA promises 1 ulp):
test_exp2_of_integers_is_exact shows it on the decode partials, first in the file."""

import pytest
import torch

import attn_exact as X

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
SLACK = 37
FORMS = [("PRE", 0.0), ("c=1", X.G_LN2)]
TOTALS = {"elems": 0, "bad": 0, "allowed": 0, "cases": 0}


@pytest.fixture(scope="module")
def ops():
    from evo_amd.ops import HipOps
    yield HipOps()
    print(f"\n[attn graded] module total: {TOTALS['cases']} comparisons, {TOTALS['elems']} elements, {TOTALS['bad']} outside the rule, "
          f"{TOTALS['allowed']} on the boundary allowance")


def _poisoned(shape, dtype=BF):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(-1).view(torch.uint8).fill_(0xFF)
    return t


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _twice(fn):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for x, y in zip(a, b) if isinstance(a, tuple) else ((a, b),):
        assert torch.equal(_bits(x), _bits(y)), "two launches differ"
    return a


def _dims(n):
    return X.DIMS2[n % 3]


def _judge(got, c, what, n_splits=0):
    ref = X.expected_graded(c["e"], c["mu"], c["v"], c["mult"])
    allow = X.graded_allow(c["mult"], c["stair"], n_splits)
    ver = X.judge_graded(got, ref, allow)
    TOTALS["elems"] += ver.n_elems
    TOTALS["bad"] += ver.n_bad
    TOTALS["allowed"] += ver.n_allowed
    TOTALS["cases"] += 1
    print(f"[attn graded] {what}: {ver}")
    if not ver.ok:
        bad = ver.bad.nonzero()[:6].tolist()
        b, i = bad[0] if bad else (0, 0)
        g, r = got[b, i, 0].double(), ref[b, i, 0]
        d = ((g - r.float().bfloat16().double()) != 0).nonzero().flatten()[:6]
        raise AssertionError(f"{what}: {ver}; first bad rows (b, query) {bad}; row ({b}, {i}) head 0 mu {int(c['mu'][b, i])} dims {d.tolist()} "
                             f"got {g[d].tolist()} ref {r[d].tolist()} old pin would flag {X.old_pin_count(got, ref)}")
    return ver


# ================================================================================================ exp2 of integers
EXP2_MAXIMA = [-100, -64, -33, -1, 0, 31, 65, 100]


@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_exp2_of_integers_is_exact(ops, form):
    """One split, two keys at exponents {M, M - n}: part_ml must hold (M, 1 + 2^-n) and part_o (s, s 2^-n) bit for bit for n = 1 .. 23 and
    the maximum M at eight values across [-100, 100] -- v_exp_f32(-n) == 2^-n exactly, with no dependence on where the maximum lies."""
    ns = list(range(1, 24))
    rows = [(M, n) for M in EXP2_MAXIMA for n in ns]
    B = len(rows)
    e = torch.tensor([[M, M - n] for M, n in rows], dtype=torch.int64, device=DEV)
    q = torch.zeros(B, 1, 1, 128, dtype=torch.float64, device=DEV)
    k = torch.zeros(B, 2, 1, 128, dtype=torch.float64, device=DEV)
    k[..., 5] = torch.div(e, 16, rounding_mode="floor").double()[:, :, None]
    k[..., 77] = (e % 16).double()[:, :, None]
    q[..., 5], q[..., 77] = 16.0, 1.0
    v = X.v_hist(B, 2, 1, DEV)
    s = X.head_factor(B, 1, DEV).flatten().float().cpu()
    o, part_o, part_ml = _decode(ops, q.to(BF), k.to(BF), v, [1] * B, 1, form[1])
    n_t = torch.tensor([n for _, n in rows], dtype=torch.float64)
    want_m = torch.tensor([float(M) for M, _ in rows])
    want_l = (1.0 + torch.exp2(-n_t)).float()
    got_m, got_l = part_ml[:, 0, 0, 0].cpu(), part_ml[:, 0, 0, 1].cpu()
    dev = (got_l.double() - want_l.double()) / 2.0 ** -24
    print(f"[attn graded] exp2 {form[0]}: {B} (maximum, n) pairs, l == 1 + 2^-n in {int((got_l == want_l).sum())}, worst deviation "
          f"{float(dev.abs().max()):.3f} units of 2^-24")
    bad = (got_l != want_l).nonzero().flatten().tolist()
    assert torch.equal(got_m, want_m), "a split's m is not its largest exponent"
    assert not bad, f"v_exp_f32 is not exact on integers: (maximum, n, deviation in 2^-24) {[(rows[i][0], rows[i][1], float(dev[i])) for i in bad[:12]]}"
    want_o = torch.zeros(B, 128)
    want_o[:, 0], want_o[:, 1] = s, s * torch.exp2(-n_t).float()
    assert torch.equal(_bits(part_o[:, 0, 0].cpu()), _bits(want_o))


# ================================================================================================ prefill
def _attention(ops, q, k, v, q_pos0, scale, w64=True):
    """evo_attn_fwd_causal_bf16 as HipOps.attention calls it (the V^T workspace for query ranges beyond 128 rows), at a given
    softmax_scale, into a poisoned output."""
    from evo_amd.ops import _check, _ptr, _stream
    B, Tq, H, hd = q.shape
    Tk = k.shape[1]
    o = _poisoned((B, Tq, H, hd))
    vt = _poisoned((B, H, hd, (Tk + 63) // 64 * 64)) if (Tq > 128 and w64) else None
    _check(ops.lib.evo_attn_fwd_causal_bf16(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), B, H, Tq, Tk, int(q_pos0),
        q.stride(0), q.stride(1), q.stride(2), k.stride(0), k.stride(1), k.stride(2),
        v.stride(0), v.stride(1), v.stride(2), scale, _ptr(vt), _stream()), "evo_attn_fwd_causal_bf16")
    return o


def _prefill(ops, c, q_pos0, scale, w64=True):
    """q / k / v as thirds of a packed qkv where the shapes allow it, else k / v as views of a cache whose rows behind Tk are 0xFF."""
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
    return _twice(lambda: _attention(ops, qq, kk, vv, q_pos0, scale, w64))


def _prefill_cases(ops, kind, shape, B, H, n, variants=X.G_VARIANTS, w64=True):
    for i, stair in enumerate(variants):
        c = X.graded_prefill(shape, B, H, _dims(n + i), stair, DEV)
        for name, scale in FORMS:
            got = _prefill(ops, c, shape[1], scale, w64)
            _judge(got, c, f"{kind} {stair or 'flat'} {name} B {B} H {H} Tq {shape[0]} q_pos0 {shape[1]} Tk {c['k'].shape[1]} dims {c['dims']}")


@pytest.mark.parametrize("n", range(len(X.G_W64)), ids=[f"Tq{s[0]}-p{s[1]}-d{s[2]}-B{b}H{h}" for s, b, h in X.G_W64])
def test_w64_prefill_on_graded_weights(ops, n):
    """attn_fwd_w64_kernel<PRE, false>: the reference point at 0 inside +-W_THRP, a first tile beyond -W_THRP, moves beyond +W_THRP (PRE);
    the first tile's maximum and moves beyond +W_THR (plain, c = 1); alpha = 2^-dl applied to l and O."""
    shape, B, H = X.G_W64[n]
    assert shape[0] > 128 and ops.attn_w64
    _prefill_cases(ops, "w64", shape, B, H, n)


@pytest.mark.parametrize("n", range(len(X.G_PIPE)), ids=[f"Tq{s[0]}-p{s[1]}" for s in X.G_PIPE])
def test_pipe_prefill_on_graded_weights(ops, n):
    """attn_fwd_pipe_kernel (no V^T workspace): the running maximum, alpha on every new one."""
    _prefill_cases(ops, "pipe", X.G_PIPE[n], 3, 2, n + 1, w64=False)


@pytest.mark.parametrize("n", range(len(X.G_QB128) + 1), ids=[f"Tq{s[0]}-p{s[1]}" for s in X.G_QB128 + [X.G_QB128_LONG]])
def test_qb128_prefill_on_graded_weights(ops, n):
    """attn_fwd_kernel<false>: query ranges of at most one 128-row block; flat only at 2,049 keys."""
    if n < len(X.G_QB128):
        _prefill_cases(ops, "qb128", X.G_QB128[n], 3, 2, n + 2)
    else:
        _prefill_cases(ops, "qb128", X.G_QB128_LONG, 3, 2, n + 2, variants=(None,))


# ================================================================================================ shared prefix
def _attention_prefix(ops, q, k, v, k_pre, vt_pre, scale):
    """evo_attn_fwd_prefix_bf16 as HipOps.attention_prefix calls it, at a given softmax_scale."""
    from evo_amd.ops import _check, _stream
    B, Tq, H, hd = q.shape
    P = k_pre.shape[0]
    o = _poisoned((B, Tq, H, hd))
    vt = _poisoned((B, H, hd, (Tq + 63) // 64 * 64))
    _check(ops.lib.evo_attn_fwd_prefix_bf16(
        q.data_ptr(), k.data_ptr(), v.data_ptr(), k_pre.data_ptr(), vt_pre.data_ptr(), o.data_ptr(), B, H, Tq, P,
        q.stride(0), q.stride(1), q.stride(2), k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1), v.stride(2),
        k_pre.stride(0), k_pre.stride(1), vt_pre.shape[2], scale, vt.data_ptr(), _stream()), "evo_attn_fwd_prefix_bf16")
    return o


@pytest.mark.parametrize("P,Tq", X.G_PREFIX)
def test_prefix_attention_on_graded_weights(ops, P, Tq):
    """attn_fwd_w64_kernel<PRE, SEG = true>: a level step on the P - 1 | P seam, every batch row its own suffix exponents behind the
    shared prefix; both ways to hand over the prefix's V: its own plane and the plane of a longer prefix."""
    B, H = 3, 2
    for i, stair in enumerate(X.G_VARIANTS):
        c = X.graded_prefill((Tq, P, 0), B, H, _dims(P // 64 + Tq + i), stair, DEV, P=P)
        c["v"][:, :P] = c["v"][:1, :P]                                  # (V_hist carries a factor per batch row: the prefix is row 0's)
        kvp = _poisoned((1, P + SLACK, 2, H, 128))
        kvp[0, :P, 0], kvp[0, :P, 1] = c["k"][0, :P], c["v"][0, :P]
        qkv = torch.stack([c["q"], c["k"][:, P:], c["v"][:, P:]], 2)
        kv2 = _poisoned((1, P + 128 + SLACK, 2, H, 128))
        kv2[:, :P] = kvp[:, :P]
        kv2[:, P:P + 128] = 1.0                                         # the longer prefix's own keys: finite, visible to nobody here
        plane = ops.attention_prefix_vt(kvp[0, :P, 1])
        plane2 = ops.attention_prefix_vt(kv2[0, :P + 128, 1])
        for name, scale in FORMS:
            what = f"prefix {stair or 'flat'} {name} P {P} Tq {Tq} dims {c['dims']}"
            got = _twice(lambda: _attention_prefix(ops, qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], kvp[0, :P, 0], plane, scale))
            _judge(got, c, what)
            got2 = _twice(lambda: _attention_prefix(ops, qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], kv2[0, :P, 0], plane2, scale))
            assert torch.equal(_bits(got2), _bits(got)), what + ": the longer prefix's plane"


# ================================================================================================ decode
def _decode(ops, q, k, v, positions, n_splits, scale):
    """evo_attn_decode_bf16 with caller-owned part_o / part_ml pre-filled with NaN; two launches, all three outputs bit-identical.
    -> (o [B, 1, H, 128], part_o [B, H, n_splits, 128], part_ml [B, H, n_splits, 2])"""
    from evo_amd.ops import _check, _stream
    B, _, H, hd = q.shape
    Tk = k.shape[1]
    pos = torch.tensor(positions, dtype=torch.int64, device=DEV)

    def once():
        o = _poisoned((B, 1, H, hd))
        part_o = _poisoned((B, H, n_splits, hd), torch.float32)
        part_ml = _poisoned((B, H, n_splits, 2), torch.float32)
        _check(ops.lib.evo_attn_decode_bf16(
            q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), B, H, Tk, q.stride(0), q.stride(2),
            k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1), v.stride(2), pos.data_ptr(),
            part_o.data_ptr(), part_ml.data_ptr(), n_splits, scale, _stream()), "evo_attn_decode_bf16")
        return o, part_o, part_ml
    return _twice(once)


def _default_splits(Tk):
    return min(((Tk + 63) // 64 + 3) // 4 * 4, 32)                      # HipOps._decode_splits


def _cache(c, positions, cap):
    """[B + 1, cap, 2, H, 128], 0xFF everywhere except each row's keys 0 .. position."""
    B, H = len(positions), c["k"].shape[2]
    kv = _poisoned((B + 1, cap, 2, H, 128))
    for b, p in enumerate(positions):
        kv[b, :p + 1, 0], kv[b, :p + 1, 1] = c["k"][b, :p + 1], c["v"][b, :p + 1]
    return kv


def _assert_partials(part_o, part_ml, c, positions, n_splits, what):
    """Flat cases: the fp32 partials themselves, on bit views: m the split's largest exponent, l the exact sum, part_o unnormalised."""
    want_o, want_ml = X.stream_partials_expected(c, positions, n_splits)
    got_o, got_ml = part_o.cpu(), part_ml.cpu()
    bad = (_bits(got_ml) != _bits(want_ml)).any(-1)
    assert not bool(bad.any()), f"{what}: per-split (m, l) differ at (b, h, split) {bad.nonzero()[:8].tolist()}: got {got_ml[bad][:4].tolist()} " \
                                f"want {want_ml[bad][:4].tolist()}"
    bad = (_bits(got_o) != _bits(want_o)).any(-1)
    assert not bool(bad.any()), f"{what}: part_o differs at (b, h, split) {bad.nonzero()[:8].tolist()}"


def _decode_cases():
    """(positions, stair): the long flat batch (win = 5) and the short batch under all four variants."""
    return [(X.DECODE_POSITIONS, None)] + [(X.G_DECODE_STAIR, s) for s in X.G_VARIANTS]


@pytest.mark.parametrize("ns", X.G_DECODE_SPLITS, ids=[f"splits{ns}" for ns in X.G_DECODE_SPLITS])
def test_decode_stream_on_graded_weights(ops, ns):
    """attn_decode_stream_kernel + attn_decode_combine_kernel: alpha = 2^(m_old - m_new) per half, the combine's 2^(m_s - M) per split
    (40 splits: its 32-split trips and its tail loop); on flat cases the partials are compared too."""
    H = 2
    for n, (positions, stair) in enumerate(_decode_cases()):
        cap = max(positions) + 1 + SLACK
        n_splits = _default_splits(cap) if ns is None else ns
        c = X.graded_decode(positions, H, _dims(n + n_splits), stair, DEV)
        kv = _cache(c, positions, cap)
        for name, scale in FORMS:
            what = f"decode stream {stair or 'flat'} {name} {len(positions)} rows to {max(positions)} n_splits {n_splits} dims {c['dims']}"
            o, part_o, part_ml = _decode(ops, c["q"], kv[:-1, :, 0], kv[:-1, :, 1], positions, n_splits, scale)
            _judge(o, c, what, n_splits)
            if stair is None:
                _assert_partials(part_o, part_ml, c, positions, n_splits, what)


# ================================================================================================ decode beyond 4 GiB: attn_fwd_kernel<true>
@pytest.fixture(scope="module")
def big():
    import test_gpu_attn_exact as T
    t = torch.empty((T.MFMA_TK - 1) * T.MFMA_ST + 2 * 2 * 2 * 128, dtype=BF, device=DEV)
    yield t
    del t
    torch.cuda.empty_cache()


@pytest.mark.parametrize("ns", [1, 3, 7])
def test_decode_mfma_split_kernel_on_graded_weights(ops, big, ns):
    """attn_fwd_kernel<true>, reached as tests/test_gpu_attn_exact.py reaches it (token stride 2 MiB, Tk = 2,100: 32-bit key offsets do
    not reach), MFMA_POSITIONS in its pairs; flat (win = 5)."""
    import test_gpu_attn_exact as T
    for n, positions in enumerate(T.MFMA_PAIRS):
        c = X.graded_decode(list(positions), 2, _dims(n + ns), None, DEV)
        k, v = T._big_views(big, c, positions)
        for name, scale in FORMS:
            o, _, _ = _decode(ops, c["q"], k, v, list(positions), ns, scale)
            _judge(o, c, f"decode MFMA split flat {name} positions {positions} n_splits {ns} dims {c['dims']}", ns)


# ================================================================================================ decode behind shared prompts
@pytest.mark.parametrize("sp", [(1, 1), (4, 4), (40, 8), None], ids=["1+1", "4+4", "40+8", "default"])
def test_decode_group_on_graded_weights(ops, sp):
    """attn_decode_group_kernel + attn_decode_stream_kernel + one combine (evo_attn_decode_prefix_bf16) on the concatenation [store row |
    own keys], PRE_ROW / OWN_POS / PRE_LENS of tests/test_gpu_attn_decode_prefix.py: the store part and the own part meet in the combine
    at weights 2^+-k.  Flat on both length sets; stair on (32, 64, 33), where the cut at key 64 is the last-key seam of store row 1."""
    import test_gpu_attn_decode_prefix as D
    from evo_amd.ops import _check, _stream
    H, B = D.H, len(D.PRE_ROW)
    for pl, pre_len in enumerate(D.PRE_LENS):
        R, P_cap, cap = 3, max(pre_len) + SLACK, max(D.OWN_POS) + 1 + SLACK
        n_pre, n_own = (ops._decode_splits(P_cap), ops._decode_splits(cap)) if sp is None else sp
        plen = D._plen(D.PRE_ROW, pre_len)
        total = [p + o for p, o in zip(plen, D.OWN_POS)]
        Tk = max(total) + 1
        for i, stair in enumerate(X.G_VARIANTS if max(total) < X.G_STAIR_MAX_KEYS else (None,)):
            win = X.G_WIN_STAIR if stair else X.graded_win(Tk)
            c = X.build_graded(B, H, 1, 0, Tk, _dims(i + n_pre + pl), win, stair, DEV, mult=X.decode_mult(total, Tk, DEV), row_mu=True)
            for r, lead in D._leads(D.PRE_ROW).items():                 # the lead row's prefix IS the store row
                P = pre_len[r]
                for b in range(B):
                    if D.PRE_ROW[b] == r and b != lead:
                        c["k"][b, :P], c["v"][b, :P], c["e"][b, :P] = c["k"][lead, :P], c["v"][lead, :P], c["e"][lead, :P]
            store, kv = D._place(c, D.PRE_ROW, pre_len, D.OWN_POS, P_cap, cap, R)
            k, v, ks, vs = kv[:B, :, 0], kv[:B, :, 1], store[:R, :, 0], store[:R, :, 1]
            row, ln, own = D._i64(D.PRE_ROW), D._i64(pre_len), D._i64(D.OWN_POS)
            q = c["q"]
            for name, scale in FORMS:
                def once():
                    o = _poisoned((B, 1, H, 128))
                    part_o = _poisoned((B, H, n_pre + n_own, 128), torch.float32)
                    part_ml = _poisoned((B, H, n_pre + n_own, 2), torch.float32)
                    _check(ops.lib.evo_attn_decode_prefix_bf16(
                        q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), B, H, k.shape[1], q.stride(0), q.stride(2),
                        k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1), v.stride(2), own.data_ptr(),
                        ks.data_ptr(), vs.data_ptr(), R, ks.shape[1], ks.stride(0), ks.stride(1), ks.stride(2), vs.stride(0), vs.stride(1),
                        vs.stride(2), row.data_ptr(), ln.data_ptr(), part_o.data_ptr(), part_ml.data_ptr(), n_pre, n_own, scale,
                        _stream()), "evo_attn_decode_prefix_bf16")
                    return o, part_o, part_ml
                o, _, _ = _twice(once)
                _judge(o, c, f"decode group {stair or 'flat'} {name} pre_len {pre_len} splits {n_pre}+{n_own} dims {c['dims']}", n_pre + n_own)


# ================================================================================================ paged
@pytest.mark.parametrize("pt,kind", [(64, "reversed"), (64, "random"), (256, "interleaved"), (256, "random")])
def test_decode_paged_on_graded_weights(ops, pt, kind):
    """attn_decode_paged_kernel: the stream cases through a page table; bit-identical to the contiguous sibling at the same n_splits,
    and judged on its own."""
    from paged_ref import n_pages_of, page_map, scatter, table_of
    from evo_amd.ops import _check, _stream
    H = 2
    for n, (positions, stair) in enumerate(_decode_cases()):
        B = len(positions)
        width = max(positions) // pt + 1
        ns = X.G_DECODE_SPLITS[(n + pt // 64) % 5]
        n_splits = ops._decode_splits((width + 2) * pt) if ns is None else ns
        c = X.graded_decode(positions, H, _dims(n + pt), stair, DEV)
        kvc = torch.stack([c["k"], c["v"]], 2)
        kv = _cache(c, positions, kvc.shape[1] + SLACK)
        pm = page_map(kind, B, width, seed=n, spare=3)
        n_pages = n_pages_of(B, width, 3)
        pages = scatter(kvc, pm, pt, n_pages, lengths=[p + 1 for p in positions], out=_poisoned((n_pages, pt, 2, H, 128)))
        table = table_of(pm, width + 2)
        for b, p in enumerate(positions):
            table[b, p // pt + 1:] = 0
        table = table.to(DEV)
        pos = torch.tensor(positions, dtype=torch.int64, device=DEV)
        q = c["q"]
        for name, scale in FORMS:
            def once():
                o = _poisoned((B, 1, H, 128))
                part_o, part_ml = _poisoned((B, H, n_splits, 128), torch.float32), _poisoned((B, H, n_splits, 2), torch.float32)
                _check(ops.lib.evo_attn_decode_paged_bf16(
                    q.data_ptr(), pages.data_ptr(), table.data_ptr(), o.data_ptr(), B, H, pages.shape[1], pages.shape[0], table.shape[1],
                    q.stride(0), q.stride(2), pages.stride(0), pages.stride(1), pages.stride(2), pages.stride(3), pos.data_ptr(),
                    part_o.data_ptr(), part_ml.data_ptr(), n_splits, scale, _stream()), "evo_attn_decode_paged_bf16")
                return o, part_o, part_ml
            what = f"decode paged {stair or 'flat'} {name} pt {pt} {kind} rows to {max(positions)} n_splits {n_splits}"
            o, part_o, part_ml = _twice(once)
            want, want_o, want_ml = _decode(ops, q, kv[:-1, :, 0], kv[:-1, :, 1], positions, n_splits, scale)
            assert torch.equal(_bits(o), _bits(want)), what + ": differs from evo_attn_decode_bf16"
            assert torch.equal(_bits(part_ml), _bits(want_ml)) and torch.equal(_bits(part_o), _bits(want_o)), what + ": partials differ"
            _judge(o, c, what, n_splits)


# ================================================================================================ FP8 cache
def _fp8_case(positions, H, dims, stair):
    """G on the quantisers' fixed points (tests/kv_fp8_exact.py): the digits e div 16 (-5 .. 4) and e mod 16 (0 .. 15) and V_hist's
    powers of two are e4m3 numbers under power-of-two scales; K is stored under the scale 2 in front of key 64 and 2^-2 from there on
    (two scales across the step at 64), V under s_bh 2^(hash mod 4)."""
    import kv_fp8_exact as E
    c = X.graded_decode(positions, H, dims, stair, DEV)
    B, Tk = c["k"].shape[:2]
    j = torch.arange(Tk, device=DEV)
    ks = torch.where(j < 64, 2.0, 0.25).float()[None, :, None].expand(B, Tk, H).contiguous()
    vs = X.head_factor(B, H, DEV).float()[:, :, :, 0] * E.pow2(X.mix31(E._key_index(B, Tk, H, DEV), 74) % 4)
    f = {"kb": E.f8_bytes(c["k"].float() / ks[..., None]), "ks": ks, "vb": E.f8_bytes(c["v"].float() / vs[..., None]), "vs": vs,
         "positions": list(positions)}
    assert torch.equal(E.f8_value(f["kb"]) * ks[..., None], c["k"].float()) and torch.equal(E.f8_value(f["vb"]) * vs[..., None], c["v"].float())
    c["data"], c["scale"] = E.pack(f, Tk + SLACK)
    return c


FP8_SHORT = [p for p in X.DECODE_POSITIONS if p <= 448] + [299, 447]


@pytest.mark.parametrize("ns", [1, 4, 40, None], ids=lambda ns: f"splits{ns}")
def test_decode_fp8_on_graded_weights(ops, ns):
    """attn_decode_fp8_kernel: score = dot x K scale x scale_log2, the weight multiplied by the V scale once, the same half-by-half
    (m, l, O) and the shared combine.  Positions up to 448 flat + stair, and the product shape (DECODE_POSITIONS) flat."""
    from evo_amd.ops import _check, _stream
    H = 2
    for n, (positions, stair) in enumerate([(X.DECODE_POSITIONS, None)] + [(FP8_SHORT, s) for s in X.G_VARIANTS]):
        c = _fp8_case(positions, H, _dims(n + (ns or 0)), stair)
        B, cap = len(positions), c["data"].shape[1]
        n_splits = _default_splits(cap) if ns is None else ns
        data, scale_t, q = c["data"], c["scale"], c["q"]
        pos = torch.tensor(positions, dtype=torch.int64, device=DEV)
        for name, scale in FORMS:
            def once():
                o = _poisoned((B, 1, H, 128))
                part_o, part_ml = _poisoned((B, H, n_splits, 128), torch.float32), _poisoned((B, H, n_splits, 2), torch.float32)
                _check(ops.lib.evo_attn_decode_fp8(
                    q.data_ptr(), data.data_ptr(), scale_t.data_ptr(), o.data_ptr(), B, H, cap, q.stride(0), q.stride(2),
                    data.stride(0), data.stride(1), data.stride(2), data.stride(3), scale_t.stride(0), scale_t.stride(1), scale_t.stride(2),
                    pos.data_ptr(), part_o.data_ptr(), part_ml.data_ptr(), n_splits, scale, _stream()), "evo_attn_decode_fp8")
                return o, part_o, part_ml
            o, part_o, part_ml = _twice(once)
            what = f"decode fp8 {stair or 'flat'} {name} rows to {max(positions)} n_splits {n_splits} dims {c['dims']}"
            _judge(o, c, what, n_splits)
            if stair is None:
                _assert_partials(part_o, part_ml, c, positions, n_splits, what)
