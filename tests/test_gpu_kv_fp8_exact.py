"""GPU (-m gpu): evo_attn_decode_fp8 on EXACT key sets (tests/kv_fp8_exact.py; tests/PARITY_kv_fp8.md "Exact key sets", PARITY row 22h).

Every softmax weight of these caches is exactly 1 or 0 and every dequantised value is exact, so a row's output says which (bytes, scale)
pairs it consumed: D / D' / S rows must return bf16(byte * scale) of ONE cached V row bit for bit, U rows bf16(sum of V scales per residue
class / n) (the adjacent pattern only within 2^-21 |ref| of a rounding boundary, at most 0.1 % of a case: attn_exact.judge, unchanged).
No tensor-wide term.  Launches go through the C entry with caller-owned NaN-filled part_o / part_ml; every launch is issued twice and the
pair (o, part_o, part_ml) must be bit-identical.  Under U part_ml is (0, the split's key count) or (-inf, 0) by value: the interleaved
block-to-split map, read back.  The expected values come from attn_exact.expected on the dequantised designs, never from the kernel.

Plain form: the kernel subtracts from a key's exponent the very fp32 maximum it took from the same numbers, so the winner's exponent is
exactly 0, P = l = 1 and no adjacent-pattern exception applies; none is granted here."""
import ctypes
import math

import pytest
import torch

import attn_exact as X
import kv_fp8_exact as E
from test_kv_fp8_exact_host import CAUGHT, EVERY_SPLITS, TABLE_SPLITS, table_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
SLACK = 37                               # cache rows behind the last key: NaN bytes with NaN scales
EVERY_B = 448


@pytest.fixture(scope="module")
def ops():
    from evo_amd.ops import HipOps
    return HipOps()


@pytest.fixture(scope="module")
def shared():
    """Cases built once per module (inputs, packed cache, reference) and shared by the tests that use them, unchanged."""
    store = {}
    yield store
    store.clear()
    torch.cuda.empty_cache()


def _poisoned(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(-1).view(torch.uint8).fill_(0xFF)
    return t


def _launch(ops, q, data, scale, B, H, Tk, positions, n_splits, pre):
    """The C entry as HipOps.attention_decode_fp8 calls it, with caller-owned part_o / part_ml (and o) pre-filled with NaN; two launches, all
    three outputs bit-identical.  positions None: the scalar form (dyn_pos null, every row sees Tk keys).  -> (o, part_ml)"""
    from evo_amd.ops import _check, _stream
    pos = None if positions is None else torch.tensor(positions, dtype=torch.int64, device=DEV)
    outs = []
    for _ in range(2):
        o = _poisoned((B, 1, H, 128), BF)
        part_o = _poisoned((B, H, n_splits, 128), torch.float32)
        part_ml = _poisoned((B, H, n_splits, 2), torch.float32)
        _check(ops.lib.evo_attn_decode_fp8(
            q.data_ptr(), data.data_ptr(), scale.data_ptr(), o.data_ptr(), B, H, Tk, q.stride(0), q.stride(2),
            data.stride(0), data.stride(1), data.stride(2), data.stride(3), scale.stride(0), scale.stride(1), scale.stride(2),
            None if pos is None else pos.data_ptr(), part_o.data_ptr(), part_ml.data_ptr(), n_splits,
            0.0 if pre else 1.0 / math.sqrt(128), _stream()), "evo_attn_decode_fp8")
        outs.append((o, part_o, part_ml))
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(E.bits(a), E.bits(b)), "two launches differ"
    return outs[0][0], outs[0][2]


def _assert_split_counts(part_ml, n_keys, n_splits, what):
    """U: every exponent is 0 and every weight 1, so a split's (m, l) is (0, the number of keys it took) or (-inf, 0) when it took none."""
    B, H = part_ml.shape[:2]
    want = torch.empty(B, H, n_splits, 2, dtype=torch.float32)
    for b, n in enumerate(n_keys):
        cnt = torch.tensor(E.stream_split_counts(n, n_splits), dtype=torch.float32)
        want[b, :, :, 0] = torch.where(cnt > 0, 0.0, float("-inf"))[None, :]
        want[b, :, :, 1] = cnt[None, :]
    got = part_ml.cpu()
    bad = (got != want).any(-1)
    assert not bool(bad.any()), f"{what}: per-split (m, l) differ from the interleaved partition at (b, h, split) {bad.nonzero()[:8].tolist()}: " \
                                f"got {got[bad][:4].tolist()} want {want[bad][:4].tolist()}"


def _case(shared, key, design, positions, H, dims, cap, **kw):
    """A built case with its packed cache and its reference, shared under `key`."""
    if key not in shared:
        c = E.build(design, positions, H, dims, DEV, **kw)
        c["data"], c["scale"] = E.pack(c, cap)
        c["ref"] = E.expected(c["lev"], c["v"], c["mult"])
        del c["kb"], c["vb"], c["ks"], c["vs"]
        shared[key] = c
    return shared[key]


def _run(ops, c, n_splits, pre, what, n_keys=None):
    """Launch twice, judge every element; under U the partials too.  -> (o, part_ml)"""
    B, _, H, _ = c["q"].shape
    positions = c["positions"] if n_keys is None else None
    Tk = c["data"].shape[1] if n_keys is None else n_keys
    o, part_ml = _launch(ops, c["q"], c["data"], c["scale"], B, H, Tk, positions, n_splits, pre)
    ver = E.judge(o, *c["ref"])
    what = f"{what} {c['design']}{' noncanon' if c['noncanon'] else ''} {'PRE' if pre else 'plain'} n_splits {n_splits} dims {c['dims']}"
    print(f"[kv_fp8 exact] {what}: {ver}")
    assert ver.ok, f"{what}: {ver}; first bad rows (b, query) {ver.bad.nonzero()[:8].tolist()}"
    if c["design"] != "U":
        single = c["ref"][1]
        want = c["ref"][0].to(BF)
        assert torch.equal(E.bits(o)[single], E.bits(want)[single]), what          # no element left out
    else:
        _assert_split_counts(part_ml, [p + 1 for p in c["positions"]] if n_keys is None else [n_keys] * B, n_splits, what)
    return o, part_ml


# (design, non-canonical K storage): U has no key levels to store differently
VARIANTS = [("U", False), ("D", False), ("D", True), ("D'", False), ("D'", True), ("S", False), ("S", True)]


# ================================================================================================ every position
@pytest.mark.parametrize("ns", EVERY_SPLITS, ids=[f"splits{ns}" for ns in EVERY_SPLITS])
def test_every_position_1_to_448(ops, shared, ns):
    """B = 448, row b at position b: n_keys takes EVERY value 1 .. 448 (n_my 1 .. 14 at one split: every residue mod 3 with and without the
    dropped second half, every ragged remainder mod 32 and mod 64); H = 2, cache [449, 485, 2, 2, 128].  3 and 5 splits leave waves with
    split >= n_splits in the last workgroup, 40 is more splits than blocks and runs the combine's 32-split trip and its tail."""
    positions = list(range(EVERY_B))
    planted = E.planted_for(positions, EVERY_SPLITS)
    for i, (design, nc) in enumerate(VARIANTS):
        c = _case(shared, ("every", design, nc), design, positions, 2, E.DIMSETS[i % 4], EVERY_B + SLACK, noncanon=nc,
                  planted=planted if design == "S" else None)
        for pre in (False, True):
            _run(ops, c, ns, pre, "every position")


@pytest.mark.parametrize("n_keys", [1, 32, 33, 64, 65, 96, 97, 193])
def test_scalar_form(ops, n_keys):
    """dyn_pos null, Tk = n_keys inside a larger cache: both rows see exactly n_keys keys; canaries fill the last half, NaN lies behind."""
    B, H, cap = 2, 2, 193 + SLACK
    positions = [n_keys - 1] * B
    planted = E.planted_for(positions, (1, 3))
    for i, (design, nc) in enumerate((("U", False), ("D", True), ("D'", False), ("S", True))):
        c = E.build(design, positions, H, E.DIMSETS[(i + n_keys) % 4], DEV, noncanon=nc, planted=planted if design == "S" else None)
        c["data"], c["scale"] = E.pack(c, cap, n_keys=n_keys)
        c["ref"] = E.expected(c["lev"], c["v"], c["mult"])
        for ns in (1, 3):
            for pre in (False, True):
                _run(ops, c, ns, pre, f"scalar form {n_keys} keys", n_keys=n_keys)


# ================================================================================================ the product's shapes
def _default_splits(Tk):
    return min(((Tk + 63) // 64 + 3) // 4 * 4, 32)                      # HipOps._decode_splits


@pytest.mark.parametrize("ns", X.DECODE_SPLITS, ids=[f"splits{ns}" for ns in X.DECODE_SPLITS])
def test_product_shapes(ops, shared, ns):
    """Positions {0, 1, 31, 32, 33, 63, 64, 65, 127, 128, 2080, 8228} mixed in one batch, H = 2 (four-digit keys)."""
    positions = X.DECODE_POSITIONS
    cap = max(positions) + 1 + SLACK
    n_splits = _default_splits(cap) if ns is None else ns
    assert cap * 2 * 2 * 128 < 0xffffffff
    planted = E.planted_for(positions, [_default_splits(cap) if s is None else s for s in X.DECODE_SPLITS])
    for i, (design, nc) in enumerate((("U", False), ("D", True), ("D'", True), ("S", False), ("S", True))):
        c = _case(shared, ("product", design, nc), design, positions, 2, E.DIMSETS[(i + 1) % 4], cap, noncanon=nc,
                  planted=planted if design == "S" else None)
        for pre in (False, True):
            _run(ops, c, n_splits, pre, "product shapes")


def test_product_shapes_at_32_heads(ops):
    """H = 32: the head stride of the data (128 bytes inside a 8 KiB token) and of the scales (cap floats)."""
    positions, H = [0, 31, 64, 65, 2080], 32
    cap = max(positions) + 1 + SLACK
    planted = E.planted_for(positions, (32,))
    for i, (design, nc) in enumerate((("U", False), ("D", True), ("S", True))):
        c = E.build(design, positions, H, E.DIMSETS[(i + 2) % 4], DEV, noncanon=nc, planted=planted if design == "S" else None)
        c["data"], c["scale"] = E.pack(c, cap)
        c["ref"] = E.expected(c["lev"], c["v"], c["mult"])
        for pre in (False, True):
            _run(ops, c, _default_splits(cap), pre, "H = 32")


@pytest.mark.parametrize("design", ["U", "D"])
def test_long_cache(ops, design):
    """cap = 131,072, H = 2, positions 0 / 70,000 / 131,071: U on the alternating-sign values, D on five-digit keys (non-canonical)."""
    positions, H, cap = X.LONG_POSITIONS, 2, X.LONG_CAP
    assert cap * 2 * H * 128 < 0xffffffff and E.n_digits(cap) == 5
    c = E.build(design, positions, H, E.DIMSETS[0], DEV, noncanon=design == "D", alt=True, Tk=cap)
    c["data"], c["scale"] = E.pack(c, cap)
    c["ref"] = E.expected(c["lev"], c["v"], c["mult"])
    del c["kb"], c["vb"], c["ks"], c["vs"]
    for pre in (False, True):
        _run(ops, c, _default_splits(cap), pre, "long")


# ================================================================================================ defects
def test_the_outputs_differ_from_every_caught_defect(ops, shared):
    """On the every-position batch (PRE, one and three splits) the kernel's (o, part_ml) EQUAL the emulation's without a defect and differ
    from the emulation's with each defect on every design the host table (tests/test_kv_fp8_exact_host.py CAUGHT) says catches it."""
    positions = list(range(EVERY_B))
    cases = table_cases(positions, DEV, SLACK)
    for ns in TABLE_SPLITS:
        for letter, c in cases.items():
            got = _launch(ops, c["q"], c["data"], c["scale"], EVERY_B, 2, EVERY_B + SLACK, positions, ns, True)
            good = E.emulate(c["q"], c["data"], c["scale"], positions, ns, True)
            assert not E.differs(got, good), f"{letter} n_splits {ns}: the kernel differs from the emulation without a defect"
            for d in E.ALL_DEFECTS:
                if letter in CAUGHT[E.defect_id(d)][ns]:
                    bad = E.emulate(c["q"], c["data"], c["scale"], positions, ns, True, defect=d)
                    assert E.differs(got, bad), f"{letter} n_splits {ns}: the kernel's output equals defect {E.defect_id(d)}'s"


# ================================================================================================ the largest admissible offset
BIG_ST = E.largest_token_stride()
BIG_PAIRS = [(0, 2099), (2050, 63)]


def _big_entry_code(ops, d_st):
    """The entry's host check alone: B = 0 never launches, so probe with real-looking arguments that fail only on the offset rule."""
    one = ctypes.c_void_p(16)
    return ops.lib.evo_attn_decode_fp8(one, one, one, one, 2, 2, E.BIG_TK, 768, 128, 512, d_st, 256, 128, 4 * E.BIG_TK, 2 * E.BIG_TK, E.BIG_TK,
                                       None, one, one, 1, ctypes.c_float(0.0), None)


@pytest.fixture(scope="module")
def big():
    """ONE allocation of about 4 GiB, never filled: tokens BIG_ST bytes apart, [B = 2, 2, H = 2, 128] bytes inside a token's slot."""
    return torch.empty((E.BIG_TK - 1) * BIG_ST + 2 * 2 * 2 * 128, dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("ns", [1, 7])
def test_largest_admissible_offset(ops, big, ns):
    """Tk = 2,100 keys at the largest token stride the entry admits (2,045,216 bytes: Tk * d_st = 4,294,953,600 <= 2^32 - 2); positions
    (0, 2,099) and (2,050, 63); only the rows up to a row's position are ever written (the rest of the 4 GiB is whatever it was).

    Address arithmetic, read before the first run (csrc/kv_fp8.hip): kp = data + bat * d_sb + head * d_sh and vp = kp + d_sw are 64-bit
    pointers; a lane's offset is (uint32_t)key * tst + dco with key <= min(n_keys, Tk) - 1 <= 2,099 after the clamp, tst = (uint32_t)d_st =
    2,045,216 (d_st < 2^32 since Tk * d_st < 2^32) and dco = 16 dc <= 112: at most 2,099 * 2,045,216 + 112 = 4,292,908,496 < 2^32, so no
    product wraps, and the 16 bytes read end at most at byte (Tk - 1) d_st + 512 + 256 + 128 + 128 of the allocation -- its size.  The scale
    reads are 64-bit: sp + min(key, n_keys - 1).  One stride step (16 bytes) further, Tk * d_st = 4,294,987,200 >= 2^32 - 1: refused."""
    assert E.BIG_TK * BIG_ST <= 0xffffffff - 1 and E.BIG_TK * (BIG_ST + 16) >= 0xffffffff and BIG_ST % 16 == 0
    assert _big_entry_code(ops, BIG_ST + 16) == -1
    B, H = 2, 2
    view = big.as_strided((B, E.BIG_TK, 2, H, 128), (2 * H * 128, BIG_ST, H * 128, 128, 1), 0)
    assert (E.BIG_TK - 1) * BIG_ST > 0xffe00000                        # the last key lies 2 MiB below the 4 GiB offset
    for positions in BIG_PAIRS:
        planted = E.planted_for(positions, (1, 7))
        for i, (design, nc) in enumerate((("U", False), ("D", True), ("S", True))):
            c = E.build(design, list(positions), H, E.DIMSETS[(i + ns) % 4], DEV, noncanon=nc, planted=planted if design == "S" else None)
            data, scale = E.pack(c, E.BIG_TK)
            for b, p in enumerate(positions):
                view[b, :p + 1] = data[b, :p + 1]
            c["data"], c["scale"] = view, scale[:B].contiguous()
            c["ref"] = E.expected(c["lev"], c["v"], c["mult"])
            for pre in (False, True):
                _run(ops, c, ns, pre, f"largest offset, positions {positions}")


# ================================================================================================ write path -> read path
@pytest.mark.parametrize("T0", [1, 63, 65])
def test_the_reader_consumes_what_the_writers_wrote(ops, T0):
    """The cache is built the way the product builds it: evo_kv_quant_fp8 stores T0 + b tokens of row b from strided thirds of a packed
    qkv, then one evo_rope_append_decode_fp8 per token (inv_freq = 0: cos = 1, sin = 0, the rotation is the identity at any position;
    q_scale = 1), every row at its own position, until the longest row holds 130 tokens.  After every append one evo_attn_decode_fp8 must
    return `expected` on the ORIGINAL bf16 rows (kv_fp8_exact.write_path_rows: they survive the rule bit for bit), and the q left in qkv is
    the q put in: the row the writers wrote for (b, token, plane, head) is the row, with the scale, the reader uses for that key."""
    from evo_amd.sh.cache import Fp8KV
    B, H, T = 4, 2, 130
    cap = T + SLACK
    q, k, v, lev = E.write_path_rows(B, T, H, DEV)
    kv = Fp8KV(torch.full((B + 1, cap, 2, H, 128), E.NAN_BYTE, dtype=torch.uint8, device=DEV),
               torch.full((B + 1, 2, H, cap), float("nan"), dtype=torch.float32, device=DEV))
    for b in range(B):
        n = T0 + b
        qkv = torch.stack([torch.zeros_like(k[b:b + 1, :n]), k[b:b + 1, :n], v[b:b + 1, :n]], 2)
        ops.kv_quant_fp8(qkv[:, :, 1], qkv[:, :, 2], Fp8KV(kv.data[b:b + 1], kv.scale[b:b + 1]), t0=0)
    inv = torch.zeros(64, dtype=torch.float32, device=DEV)
    rows = torch.arange(B, device=DEV)
    n_bad = n_allowed = n_elems = 0
    for step in range(T - (T0 + B - 1)):
        positions = [T0 + b + step for b in range(B)]
        pos = torch.tensor(positions, dtype=torch.int64, device=DEV)
        qkv = torch.stack([q[:, 0], k[rows, pos], v[rows, pos]], 1)[:, None].contiguous()          # [B, 1, 3, H, 128]
        put = qkv.clone()
        ops.rope_append_decode_fp8(qkv, kv.rows(B), pos, inv, 1.0, q_scale=1.0)
        assert torch.equal(E.bits(qkv), E.bits(put)), f"T0 {T0} step {step}: qkv changed under the identity rotation"
        pre, ns = bool(step % 2), (None, 1, 3)[step % 3]
        outs = [ops.attention_decode_fp8(qkv[:, :, 0], kv.rows(B), pos=pos, n_splits=ns, prescaled=pre) for _ in range(2)]
        assert torch.equal(E.bits(outs[0]), E.bits(outs[1])), "two launches differ"
        ver = E.judge(outs[0], *E.expected(lev, v, E.decode_mult(positions, T, DEV)))
        assert ver.ok, f"T0 {T0} step {step} positions {positions} n_splits {ns} {'PRE' if pre else 'plain'}: {ver}"
        n_bad, n_allowed, n_elems = n_bad + ver.n_bad, n_allowed + ver.n_allowed, n_elems + ver.n_elems
    # nothing but the written rows left their poison, and the spare row none
    assert bool((kv.data[B] == E.NAN_BYTE).all()) and bool(torch.isnan(kv.scale[B]).all())
    for b in range(B):
        assert bool((kv.data[b, positions[b] + 1:] == E.NAN_BYTE).all()) and bool(torch.isnan(kv.scale[b, :, :, positions[b] + 1:]).all())
        assert not bool(torch.isnan(kv.scale[b, :, :, :positions[b] + 1]).any())
    print(f"[kv_fp8 exact] write path -> read path T0 {T0}: {n_bad} mismatching of {n_elems} elements, {n_allowed} on the boundary allowance")
