"""CPU: the exact FP8-cache designs of tests/kv_fp8_exact.py are pinned to the OPERATION (the project's fp64 oracle op on the dequantised
cache), the plain-torch emulation of attn_decode_fp8_kernel's walk reproduces them bit for bit at the shapes tests/test_gpu_kv_fp8_exact.py
runs, and every defect of the list is shown to be caught (differing bits) by named designs -- the table CAUGHT below, which the GPU module
imports and holds the kernel's output against.

Shapes shrunk for the CPU (everything else is the GPU module's): the every-position batch holds rows 0 .. 223 instead of 0 .. 447 (n_my
1 .. 7 at one split: still every residue mod 3 with and without the dropped half and every ragged remainder; row b's data does not depend
on the batch size, so the 448-row batch catches at least what this one does); the long cache holds 65,664 keys at H = 1 with positions
0 / 35,000 / 65,663 (still five-digit keys) instead of 131,072 at H = 2; the H = 32 case is not emulated here."""
import pytest
import torch

import attn_exact as X
import kv_fp8_exact as E
from oracle_ops import OracleOps
from test_kv_fp8_host import dequant, quant_rule

BF = torch.bfloat16
SLACK = 37
EVERY_SPLITS = [1, 2, 3, 5, 8, 40]
EVERY_B_CPU = 224
VARIANTS = [("U", False), ("D", False), ("D", True), ("D'", False), ("D'", True), ("S", False), ("S", True)]

# ------------------------------------------------------------------------------------------------ the defect table
# defect -> {n_splits: the designs whose (o, part_ml) differ from the defect-free emulation's}, on the every-position batch, PRE, with
# U canonical and D / S in the non-canonical K storage (`table_cases`).  "." = not caught there.  What the table says:
#   kscale    q = 0 under U: no K scale reaches a U output.  D / S: a level moves by a power of two, another key wins.
#   vscale    U sees every key's scale; D / S see the winner's (+1 at a ragged end re-reads the clamped last key: 7 rows of D differ).
#   le        the doubled last key moves a U count; under D / S the winner is doubled in numerator and denominator alike -- only part_ml (l = 2).
#   keep      NEUTRAL, by derivation and by test: a kept half lies wholly beyond the keys, its loads are clamped to the last key (finite),
#             every score is masked to -inf, so m is unchanged, alpha = 2^0 = 1 and every weight 2^-inf = 0.  No design can see it in a value;
#             it costs eight requests.  test_the_kept_half_is_value_neutral asserts the equality; the GPU run has nothing to distinguish.
#   map       the output of an exact design does not depend on the partition (every sum is exact); part_ml does, from the first split
#             count at which the two maps differ (3 splits; at 1 split they coincide).
#   noalpha   under U every alpha is 1.
TABLE_SPLITS = (1, 3)
CAUGHT = {
    "kscale+1": {1: ".DS", 3: ".DS"},
    "kscale-1": {1: ".DS", 3: ".DS"},
    "vscale+1": {1: "UDS", 3: "UDS"},
    "vscale-1": {1: "UDS", 3: "UDS"},
    "kforv": {1: "UDS", 3: "UDS"},
    "head": {1: "UDS", 3: "UDS"},
    "planes": {1: "UDS", 3: "UDS"},
    "le": {1: "UDS", 3: "UDS"},
    "keep": {1: "...", 3: "..."},
    "ring": {1: "UDS", 3: "UDS"},
    "skip+0": {1: "UDS", 3: "UDS"},
    "skip+1": {1: "UDS", 3: "UDS"},
    "skip+2": {1: "UDS", 3: "UDS"},
    "map": {1: "...", 3: "UDS"},
    "noalpha": {1: ".DS", 3: ".DS"},
    "chunk": {1: "UDS", 3: "UDS"},
}
NEUTRAL = {"keep"}


def table_cases(positions, device, slack=SLACK):
    """{"U" / "D" / "S": case with its packed cache} on an every-position batch -- the cases the table speaks about, on any device."""
    planted = E.planted_for(positions, EVERY_SPLITS)
    out = {}
    for i, (letter, nc) in enumerate((("U", False), ("D", True), ("S", True))):
        c = E.build(letter, positions, 2, E.DIMSETS[(i + 1) % 4], device, noncanon=nc, planted=planted if letter == "S" else None)
        c["data"], c["scale"] = E.pack(c, len(positions) + slack)
        out[letter] = c
    return out


@pytest.fixture(scope="module")
def every():
    """The every-position cases (CPU rows 0 .. 223), built once: {(design, noncanon): case with cache and reference}."""
    positions = list(range(EVERY_B_CPU))
    planted = E.planted_for(positions, EVERY_SPLITS)
    out = {}
    for i, (design, nc) in enumerate(VARIANTS):
        c = E.build(design, positions, 2, E.DIMSETS[i % 4], noncanon=nc, planted=planted if design == "S" else None)
        c["data"], c["scale"] = E.pack(c, EVERY_B_CPU + SLACK)
        c["ref"] = E.expected(c["lev"], c["v"], c["mult"])
        out[(design, nc)] = c
    return out


def _close(a, b):
    """1e-12 relative; an element whose winner holds byte +0 is held to 1e-12 of the smallest nonzero magnitude a design can hold (2^-29):
    the oracle's weights of the losing keys are e^-181 and smaller, not 0."""
    return bool(((a - b).abs() <= 1e-12 * b.abs().clamp_min(2.0 ** -29)).all())


def _exact(c, n_splits, pre, n_keys=None):
    """emulate(defect=None) against bf16(expected): -> elements on the boundary allowance (D / D' / S: none may differ at all)."""
    o, _ = E.emulate(c["q"], c["data"], c["scale"], None if n_keys else c["positions"], n_splits, pre, n_keys=n_keys)
    ver = E.judge(o, *c["ref"])
    assert ver.ok and ver.n_bad == 0 and ver.n_adjacent == 0, (c["design"], c["noncanon"], n_splits, pre, ver)
    if c["design"] != "U":
        single = c["ref"][1]
        assert torch.equal(E.bits(o)[single], E.bits(c["ref"][0].to(BF))[single])
        assert c["design"] == "S" or bool(single.all())
    return ver.n_allowed


# ------------------------------------------------------------------------------------------------ closed forms vs the oracle op
@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("design,nc", VARIANTS)
def test_closed_forms_are_the_fp64_softmax_of_the_dequantised_cache(design, nc, pre):
    """expected() on the dequantised design == OracleOps.attention_decode in fp64 on the same dequantised inputs to 1e-12: plain form with its
    real scale (the oracle's 1 / sqrt(128)) and PRE (the scores are log2 exponents: q / c gives the oracle the same softmax)."""
    pos = [0, 1, 31, 32, 33, 63, 64, 65, 200]
    c = E.build(design, pos, 2, E.DIMSETS[1], noncanon=nc, planted=E.planted_for(pos, (1, 3)) if design == "S" else None)
    ref, single = E.expected(c["lev"], c["v"], c["mult"])
    q = c["q"].double() / X.C_LOG2 if pre else c["q"].double()
    want = OracleOps().attention_decode(q, E.dequantised_keys(c).double(), c["v"].double(), torch.tensor(pos))
    assert _close(ref, want)
    assert bool(single.all()) == (design in ("D", "D'"))
    if design == "S":
        assert bool(single.any()) and bool((~single).any())           # both V[t_m] rows and U means in front of t_1 occur
    # the non-canonical storage leaves the dequantised keys what the canonical one holds
    if nc:
        plain = E.build(design, pos, 2, E.DIMSETS[1], planted=c["planted"])
        assert torch.equal(E.dequantised_keys(c), E.dequantised_keys(plain)) and not torch.equal(c["kb"], plain["kb"])
        assert sorted(c["ks"].unique().tolist()) == [2.0 ** t for t in range(-3, 4)]


def test_the_designs_are_what_they_say():
    pos = list(range(0, 300, 7))
    u = E.build("U", pos, 2, E.DIMSETS[0])
    d = E.build("D", pos, 2, E.DIMSETS[0], noncanon=True)
    for c in (u, d):
        assert not bool(((c["kb"] & 0x7f) == 0x7f).any()) and not bool(((c["vb"] & 0x7f) == 0x7f).any())          # no NaN byte
        assert bool(torch.isfinite(c["v"].float()).all())
    assert not bool(u["q"].any()) and bool((u["kb"] != 0).any())
    # U values: one nonzero per key, byte 1.0, four different scales per (b, h); alt: both signs
    assert torch.equal((u["vb"] != 0).sum(-1), torch.ones_like(u["vb"][..., 0], dtype=torch.int64)) and set(u["vb"].unique().tolist()) == {0, 0x38}
    assert len((u["vs"][0, :, 0]).unique()) == 4
    assert set(E.build("U", [299], 1, E.DIMSETS[0], alt=True)["vb"].unique().tolist()) == {0, 0x38, 0xb8}
    # D values: hashed patterns of both signs with subnormals (exponent field 0) and 41 different scales
    vb = d["vb"]
    assert bool((vb >= 0x81).any()) and bool(((vb & 0x78) == 0).any()) and not bool((vb == 0x80).any()) and len(vb.unique()) == 253
    assert len(d["vs"].unique()) == 41 and float(d["vs"].min()) == 2.0 ** -20 and float(d["vs"].max()) == 2.0 ** 20
    # the digits of a five-digit key and the exactness of every score
    long = E.build("D", [70000], 1, E.DIMSETS[3], noncanon=True)
    assert len(long["dims"]) == 5
    k, q = E.dequantised_keys(long).double(), long["q"].double()
    s = torch.einsum("bihd,bjhd->bhij", q, k)[0, 0, 0]
    assert torch.equal(s, (torch.arange(70001, dtype=torch.float64) * X.G))


def test_pack_puts_canaries_in_the_last_half_and_nan_behind():
    pos = [0, 30, 31, 32, 70]
    c = E.build("D", pos, 2, E.DIMSETS[2], noncanon=True)
    data, scale = E.pack(c, 71 + SLACK)
    assert data.shape == (6, 108, 2, 2, 128) and scale.shape == (6, 2, 2, 108)
    for b, p in enumerate(pos):
        n, end = p + 1, (p + 32) // 32 * 32
        assert torch.equal(data[b, :n, 0], c["kb"][b, :n]) and torch.equal(data[b, :n, 1], c["vb"][b, :n])
        assert torch.equal(scale[b, 0, :, :n], c["ks"][b, :n].T) and torch.equal(scale[b, 1, :, :n], c["vs"][b, :n].T)
        assert bool((data[b, n:end] == E.CANARY_BYTE).all()) and bool((scale[b, :, :, n:end] == E.CANARY_SCALE).all())
        assert bool((data[b, end:] == E.NAN_BYTE).all()) and bool(torch.isnan(scale[b, :, :, end:]).all())
    assert bool((data[5] == E.NAN_BYTE).all()) and bool(torch.isnan(scale[5]).all())
    assert float(torch.tensor(E.CANARY_BYTE, dtype=torch.uint8).view(E.F8).float()) == 448.0


# ------------------------------------------------------------------------------------------------ the emulation reproduces the designs
@pytest.mark.parametrize("ns", EVERY_SPLITS)
def test_emulation_is_exact_at_every_position(every, ns):
    """Rows 0 .. 223 (see the module docstring), every design and storage, plain and PRE: D / D' / S bit for bit, U without the allowance."""
    used = sum(_exact(c, ns, pre) for c in every.values() for pre in (False, True))
    print(f"[kv_fp8 exact host] every position, {ns} splits: {used} elements on the boundary allowance")
    assert used == 0


@pytest.mark.parametrize("n_keys", [1, 32, 33, 64, 65, 96, 97, 193])
def test_emulation_is_exact_in_the_scalar_form(n_keys):
    positions = [n_keys - 1] * 2
    planted = E.planted_for(positions, (1, 3))
    used = 0
    for i, (design, nc) in enumerate((("U", False), ("D", True), ("D'", False), ("S", True))):
        c = E.build(design, positions, 2, E.DIMSETS[(i + n_keys) % 4], noncanon=nc, planted=planted if design == "S" else None)
        c["data"], c["scale"] = E.pack(c, 193 + SLACK, n_keys=n_keys)
        c["ref"] = E.expected(c["lev"], c["v"], c["mult"])
        used += sum(_exact(c, ns, pre, n_keys=n_keys) for ns in (1, 3) for pre in (False, True))
    assert used == 0


def test_emulation_is_exact_at_the_products_shapes():
    """Positions {0 .. 8228} mixed, H = 2, every split count of the GPU test (the default is 32)."""
    positions = X.DECODE_POSITIONS
    cap = max(positions) + 1 + SLACK
    splits = [32 if s is None else s for s in X.DECODE_SPLITS]
    planted = E.planted_for(positions, splits)
    used = 0
    for i, (design, nc) in enumerate((("U", False), ("D", True), ("S", True))):
        c = E.build(design, positions, 2, E.DIMSETS[(i + 1) % 4], noncanon=nc, planted=planted if design == "S" else None)
        assert len(c["dims"]) == 4
        c["data"], c["scale"] = E.pack(c, cap)
        c["ref"] = E.expected(c["lev"], c["v"], c["mult"])
        used += sum(_exact(c, ns, pre) for ns in splits for pre in ((True,) if ns in (4, 64) else (False, True)))
    print(f"[kv_fp8 exact host] product shapes: {used} elements on the boundary allowance")
    assert used == 0


@pytest.mark.parametrize("design", ["U", "D"])
def test_emulation_is_exact_on_a_long_cache(design):
    """Shrunk (module docstring): 65,664 keys, H = 1, positions 0 / 35,000 / 65,663; U on the alternating-sign values, D on five-digit keys."""
    positions, cap = [0, 35000, 65663], 65664
    c = E.build(design, positions, 1, E.DIMSETS[0], noncanon=design == "D", alt=True, Tk=cap)
    assert len(c["dims"]) == 5
    c["data"], c["scale"] = E.pack(c, cap)
    c["ref"] = E.expected(c["lev"], c["v"], c["mult"])
    used = sum(_exact(c, 32, pre) for pre in (False, True))
    print(f"[kv_fp8 exact host] long {design}: {used} elements on the boundary allowance")
    assert used == 0


# ------------------------------------------------------------------------------------------------ every defect against the table
@pytest.fixture(scope="module")
def table():
    return table_cases(list(range(EVERY_B_CPU)), "cpu")


@pytest.mark.parametrize("defect", E.ALL_DEFECTS, ids=[E.defect_id(d) for d in E.ALL_DEFECTS])
def test_every_defect_is_caught_where_the_table_says(table, defect):
    name = E.defect_id(defect)
    positions = list(range(EVERY_B_CPU))
    caught_somewhere = False
    for ns in TABLE_SPLITS:
        got = ""
        for letter, c in table.items():
            good = E.emulate(c["q"], c["data"], c["scale"], positions, ns, True)
            bad = E.emulate(c["q"], c["data"], c["scale"], positions, ns, True, defect=defect)
            got += letter if E.differs(good, bad) else "."
        assert got == CAUGHT[name][ns], (name, ns, got)
        caught_somewhere |= got != "..."
    assert caught_somewhere != (name in NEUTRAL), name


def test_the_table_names_every_defect():
    assert sorted(CAUGHT) == sorted(E.defect_id(d) for d in E.ALL_DEFECTS)
    assert {d if isinstance(d, str) else d[0] for d in E.ALL_DEFECTS} == set(E.DEFECTS)
    for name, row in CAUGHT.items():
        assert set(row) == set(TABLE_SPLITS) and all(len(v) == 3 and set(v) <= set("UDS.") for v in row.values())
        assert (name in NEUTRAL) == all(v == "..." for v in row.values())


def test_the_kept_half_is_value_neutral(every):
    """Defect `keep` (the second half beyond the keys is not dropped): outputs and partials equal the defect-free walk's on every design."""
    for c in every.values():
        for ns in (1, 3):
            a = E.emulate(c["q"], c["data"], c["scale"], c["positions"], ns, False)
            b = E.emulate(c["q"], c["data"], c["scale"], c["positions"], ns, False, defect="keep")
            assert not E.differs(a, b)


def test_the_emulated_partials_are_the_split_counts(every):
    c = every[("U", False)]
    for ns in (1, 3, 40):
        _, ml = E.emulate(c["q"], c["data"], c["scale"], c["positions"], ns, True)
        for b in (0, 63, 64, 130, 223):
            cnt = torch.tensor(E.stream_split_counts(b + 1, ns), dtype=torch.float32)
            assert torch.equal(ml[b, 0, :, 1], cnt) and torch.equal(ml[b, 1, :, 0], torch.where(cnt > 0, 0.0, float("-inf")))


# ------------------------------------------------------------------------------------------------ the write path's rows
def test_write_path_rows_survive_the_rule_bit_for_bit():
    B, T, H = 4, 130, 2
    q, k, v, lev = E.write_path_rows(B, T, H)
    for x in (k, v):
        f = x.float()
        assert bool(torch.isfinite(f).all())
        m, _ = torch.frexp(f)
        assert torch.equal(m * 16, (m * 16).round())                   # at most 4 significant bits
        byts, sc = quant_rule(x)
        assert torch.equal(dequant(byts, sc).to(BF).view(torch.int16), x.view(torch.int16))
    assert bool((k.float().abs().amax(-1) > 0).all())                  # no all-zero key row
    assert not bool((v.view(torch.int16) == -32768).any()) and bool((v == 0).any()) and bool((v < 0).any())       # +0 only, both signs
    # the levels are the exact scores in units of G
    s = torch.einsum("bihd,bjhd->bhij", q.double(), k.double())
    for h in range(H):
        assert torch.equal(s[:, h, 0], lev.double() * X.G)
    assert bool((lev[0::2] > 0).all()) and bool((lev[1::2] < 0).all())
    # the winner of a row that takes the highest level is not simply the last token, and the rule gives the rows many different scales
    assert int(lev[0].argmax()) != T - 1 and int(lev[2].argmax()) != T - 1
    assert len(quant_rule(k)[1].unique()) >= 5 and len(quant_rule(v)[1].unique()) >= 10
    # the emulated reader on the rule's cache returns `expected` on the original rows, every row at its own position
    positions = [40, 129, 77, 100]
    data = torch.stack([quant_rule(k)[0], quant_rule(v)[0]], 2)
    scale = torch.stack([quant_rule(k)[1], quant_rule(v)[1]], 1).permute(0, 1, 3, 2).contiguous()
    ref = E.expected(lev, v, E.decode_mult(positions, T))
    for ns, pre in ((1, False), (3, True)):
        o, _ = E.emulate(q, data, scale, positions, ns, pre)
        ver = E.judge(o, *ref)
        assert ver.ok and ver.n_bad == 0, ver


def test_the_largest_admissible_stride():
    st = E.largest_token_stride()
    assert st == 2045216 and st % 16 == 0 and E.BIG_TK * st <= 0xffffffff - 1 < E.BIG_TK * (st + 16)
