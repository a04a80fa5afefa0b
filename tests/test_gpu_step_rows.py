"""GPU (-m gpu): the launches of the batch-invariant decode step that DESIGN.md section 25 calls row-local "by reading" -- `rmsnorm`,
`hyena_step`, rotary + append (contiguous and paged) and the decode attention at ROWINV_SPLITS splits -- held to it at kernel level.  In
every case the reference is the ONE-ROW call, and every compared tensor is compared on bit views: row b of a B-row launch must be the
bits of the launch that holds row b alone, whatever B is, wherever the row sits, whatever the other rows hold and however large the
cache is.  Values are not re-derived here, except for the attention (below); the sampler's statement of this kind is
tests/test_gpu_sample.py::test_keying_follows_stream_and_count_not_the_slot.

    rmsnorm              D in {512, 4096}, every M in 1 .. 64 (the kernel's row-to-wave map changes with M), straight and permuted rows,
                         with and without the in-place bias
    hyena_step           D = 4096 (H = 32) and 512, M in {1 .. 9, 16, 17, 32, 33, 48, 49, 64}, three consecutive steps from NON-ZERO
                         fir_state / iir_state (the start of tests/test_gpu_hyena_fused_exact.py's tail test): y and both states after
                         every step equal the one-row walks; a sentinel row behind M keeps its bits
    rope_append_decode   q and k left in qkv[b] and the kv row written at pos[b] depend on (qkv[b], pos[b]) only: B in {1, 2, 9, 33, 64},
                         the subject row first / middle / last, positions {0, 1, 8191, 131071} mixed in one batch, scaling 16, plain and
                         prescaled q; paged with 64- and 256-token pages on a scattered page map
    decode attention     n_splits = ROWINV_SPLITS (== HipOps._decode_splits(131072)), plain and prescaled queries, N(0, 1) q / k / v: the
                         subject row at position p in {0, 1, 63, 64, 2047, 2048, 2111, 8228} (fewer blocks than splits, exactly 32 blocks,
                         33 blocks, a ragged half) against the B = 1 call on a cache of capacity p + 1 -- B in {2, 5, 9, 17, 33, 64}, the
                         subject first / middle / last, capacity p + 1 / 4096 / 16384 (and 131,072 at H = 2), beside rows at position 0,
                         rows at capacity - 1 and idle rows (cache 0xFF, position 0); paged caches of 64 / 128 / 256-token pages on
                         identity, reversed and scattered maps.  H = 32 where the cache stays near 2 GiB, H = 2 otherwise.  The reference
                         itself is held against fp64 op_attention over keys [0, p] inside tests/PARITY.md row 12's pins (rel-L2 <= 4e-3,
                         |err| <= 2^-8 |ref| + 2e-2: tests/test_gpu_decode_regimes.py's rule and code)

Dispatch fact behind "any capacity": evo_attn_decode_bf16 leaves the streaming kernel for the MFMA split kernel when
Tk * k_st * 2 >= 2^32 - 1 bytes (32-bit key offsets).  In the model's cache layout k_st = 2 H 128 elements, so at H = 32 that is a
capacity of 262,144 keys -- beyond the model's 131,072.  Below it the split geometry is a function of the row's own position."""
import math
import time

import pytest
import torch

from evo_amd.sh.cache import ROWINV_SPLITS, PagedKV
from paged_ref import n_pages_of, page_map, scatter, table_of
from test_gpu_decode_regimes import _assert_decode, _judge_decode
from test_gpu_paged_kv import _inv_freq, _poisoned

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF = torch.bfloat16
PERM = torch.randperm(64, generator=torch.Generator().manual_seed(65)).tolist()
HYENA_MS = list(range(1, 10)) + [16, 17, 32, 33, 48, 49, 64]
ROPE_BS = [1, 2, 9, 33, 64]
ROPE_POSITIONS = [0, 1, 8191, 131071]
ATTN_POSITIONS = [0, 1, 63, 64, 2047, 2048, 2111, 8228]
ATTN_BS = [2, 5, 9, 17, 33, 64]
GIB = 1 << 30
TOTAL = {"launches": 0, "elements": 0, "mismatches": 0, "t0": None}
_CACHE = {}


def _ops():
    if "ops" not in _CACHE:
        from evo_amd.ops import HipOps
        _CACHE["ops"] = HipOps()
        TOTAL["t0"] = time.time()
    return _CACHE["ops"]


def _bits(t):
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _same(got, want, what):
    a, b = _bits(got), _bits(want)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    n = int((a != b).sum())
    TOTAL["elements"] += a.numel()
    TOTAL["mismatches"] += n
    assert n == 0, f"{what}: {n} of {a.numel()} bit patterns differ from the one-row call"


def _randn(*shape, seed, scale=1.0, dtype=BF):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(*shape, generator=g, device=DEV, dtype=torch.float32) * scale).to(dtype)


def _slots(B):
    return sorted({0, B // 2, B - 1})


def test_the_split_count_is_the_saturated_default():
    ops = _ops()
    assert ROWINV_SPLITS == ops._decode_splits(131072) == ops._decode_splits(1857) and ops._decode_splits(1792) < ROWINV_SPLITS


# ================================================================================================ rmsnorm
@pytest.mark.parametrize("D", [512, 4096])
def test_rmsnorm_rows_do_not_see_m_or_their_index(D):
    ops = _ops()
    x, scale, bias = _randn(64, D, seed=D + 1, scale=2.0), _randn(D, seed=D + 2, scale=0.1) + 1, _randn(D, seed=D + 3, scale=0.5)
    for bname, b in (("no bias", None), ("bias", bias)):
        def run(rows):
            xin = rows.clone()
            TOTAL["launches"] += 1
            return ops.rmsnorm(xin, b, scale, 1e-6), xin
        alone = [run(x[i:i + 1]) for i in range(64)]
        out1, x1 = torch.cat([a[0] for a in alone]), torch.cat([a[1] for a in alone])
        assert bool(torch.isfinite(out1.float()).all()) and (b is None) == torch.equal(x1, x)
        for pname, order in (("straight", list(range(64))), ("permuted", PERM)):
            xo, want_out, want_x = x[order].contiguous(), out1[order], x1[order]
            for M in range(1, 65):
                out, xin = run(xo[:M])
                _same(out, want_out[:M], f"rmsnorm D={D} {bname} {pname} M={M}: out")
                _same(xin, want_x[:M], f"rmsnorm D={D} {bname} {pname} M={M}: x (+ bias, in place)")


# ================================================================================================ hyena_step
def _hyena_data(D):
    """Random filters and NON-ZERO states for 64 rows + a sentinel row (as tests/test_gpu_hyena_fused_exact.py::_random), three steps of z."""
    g = torch.Generator().manual_seed(3000 + D)
    d = lambda t: t.to(DEV)
    fir_w = d((torch.randn(3 * D, 3, generator=g) * 0.3).bfloat16())
    fir_b = d((torch.randn(3 * D, generator=g) * 0.1).bfloat16())
    mag = 1.0 - 10.0 ** (-5.0 + 4.0 * torch.rand(D, 8, generator=g))
    ang = (torch.rand(D, 8, generator=g) * 2 - 1) * math.pi
    poles = d(torch.stack([mag * torch.cos(ang), mag * torch.sin(ang)], -1).float().contiguous())
    res = d((torch.randn(D, 8, 2, generator=g) * 0.25).float().contiguous())
    dskip = d((torch.randn(D, generator=g) * 0.5).bfloat16())
    fs = d(torch.randn(65, 3 * D, 2, generator=g).bfloat16())
    st = d(torch.view_as_complex(torch.randn(65, D, 8, 2, generator=g).contiguous()))
    zs = d(torch.randn(3, 64, 3 * D, generator=g).bfloat16())
    assert bool(fs.any()) and bool(torch.view_as_real(st).all())
    return (fir_w, fir_b, poles, res, dskip), fs, st, zs


@pytest.mark.parametrize("D", [4096, 512])
def test_hyena_step_rows_do_not_see_m(D):
    ops = _ops()
    H = D // 128
    prm, fs0, st0, zs = _hyena_data(D)
    # the 64 one-row walks: y, fir_state, iir_state after every step
    want = [[], [], []]
    for i in range(64):
        fs, st = fs0[i:i + 1].clone(), st0[i:i + 1].clone()
        for t in range(3):
            y = ops.hyena_step(zs[t, i:i + 1].contiguous(), fs, st, *prm, H)
            want[t].append((y, fs.clone(), st.clone()))
    TOTAL["launches"] += 192
    want = [tuple(torch.cat([w[k] for w in step]) for k in range(3)) for step in want]
    assert all(bool(torch.isfinite(w[0].float()).all()) for w in want)
    assert not torch.equal(want[0][1], fs0[:64]) and not torch.equal(torch.view_as_real(want[2][2]), torch.view_as_real(want[1][2]))
    for M in HYENA_MS:
        fs_all, st_all = fs0[:M + 1].clone(), st0[:M + 1].clone()                       # M rows and the sentinel row behind them
        for t in range(3):
            y = ops.hyena_step(zs[t, :M].contiguous(), fs_all[:M], st_all[:M], *prm, H)
            TOTAL["launches"] += 1
            _same(y, want[t][0][:M], f"hyena_step D={D} M={M} step {t}: y")
            _same(fs_all[:M], want[t][1][:M], f"hyena_step D={D} M={M} step {t}: fir_state")
            _same(st_all[:M], want[t][2][:M], f"hyena_step D={D} M={M} step {t}: iir_state")
        _same(fs_all[M], fs0[M], f"hyena_step D={D} M={M}: the sentinel row's fir_state")
        _same(st_all[M], st0[M], f"hyena_step D={D} M={M}: the sentinel row's iir_state")


# ================================================================================================ rotary + append
def _rope_reference(ops, sub, p, H, qs):
    """The B = 1 call on a cache of capacity p + 1 -> (qkv left behind, the kv row written at p); once per (H, p, q scale)."""
    if ("rope", H, p, qs) in _CACHE:
        return _CACHE[("rope", H, p, qs)]
    qkv = sub.clone()
    kv = _poisoned((1, p + 1, 2, H, 128))
    ops.rope_append_decode(qkv, kv, torch.tensor([p], dtype=torch.int64, device=DEV), _inv_freq(), 16.0, q_scale=qs)
    TOTAL["launches"] += 1
    if p:
        assert bool((kv[0, :p].view(torch.int16) == -1).all()), "the one-row call wrote outside its row"
    _CACHE[("rope", H, p, qs)] = (qkv, kv[0, p].clone())
    return _CACHE[("rope", H, p, qs)]


def _rope_batch(sub, B, slot, p, seed):
    """qkv [B, 1, 3, H, 128] with the subject at `slot`, and positions: the subject's p, the others ROPE_POSITIONS in turn."""
    H = sub.shape[3]
    qkv = _randn(B, 1, 3, H, 128, seed=seed)
    qkv[slot] = sub[0]
    positions = [ROPE_POSITIONS[(b + seed) % 4] for b in range(B)]
    positions[slot] = p
    return qkv, positions


@pytest.mark.parametrize("B", ROPE_BS)
def test_rope_append_depends_on_the_row_and_its_position_only(B):
    ops = _ops()
    H = 2 if B <= 33 else 1                                                             # [B, 131072, 2, H, 128] bf16: 4 GiB at the most
    cap = ROPE_POSITIONS[-1] + 1
    sub = _randn(1, 1, 3, H, 128, seed=400 + H)
    kv = torch.empty(B, cap, 2, H, 128, dtype=BF, device=DEV)
    for pre in (False, True):
        qs = ops.attn_q_scale(128) if pre else 1.0
        for p in ROPE_POSITIONS:
            want_qkv, want_row = _rope_reference(ops, sub, p, H, qs)
            assert bool(torch.isfinite(want_qkv.float()).all()) and (p == 0) == torch.equal(want_qkv[0, 0, 1], sub[0, 0, 1])
            for slot in _slots(B):
                qkv, positions = _rope_batch(sub, B, slot, p, B + slot + p)
                kv[slot, p].view(-1).view(torch.uint8).fill_(0xFF)
                ops.rope_append_decode(qkv, kv, torch.tensor(positions, dtype=torch.int64, device=DEV), _inv_freq(), 16.0, q_scale=qs)
                TOTAL["launches"] += 1
                what = f"rope_append_decode B={B} H={H} slot {slot} pos {p} prescaled={pre}"
                _same(qkv[slot], want_qkv[0], what + ": q / k left in qkv")
                _same(kv[slot, p], want_row, what + ": the kv row")
    del kv
    torch.cuda.empty_cache()


@pytest.mark.parametrize("pt", [64, 256])
@pytest.mark.parametrize("B", ROPE_BS)
def test_paged_rope_append_depends_on_the_row_and_its_position_only(B, pt):
    """A scattered map: every row owns ONE live page, the one its position falls in; every other table entry is the scrap page 0.  H = 32."""
    ops = _ops()
    H = 32
    width = ROPE_POSITIONS[-1] // pt + 1
    sub = _randn(1, 1, 3, H, 128, seed=432)
    ids = page_map("random", B, 1, seed=B + pt, spare=5)[:, 0]                           # distinct, never 0
    n_pages = n_pages_of(B, 1, 5)
    for pre in (False, True):
        qs = ops.attn_q_scale(128) if pre else 1.0
        for p in ROPE_POSITIONS:
            want_qkv, want_row = _rope_reference(ops, sub, p, H, qs)
            for slot in _slots(B):
                qkv, positions = _rope_batch(sub, B, slot, p, B + slot + p)
                table = torch.zeros(B, width, dtype=torch.int32)
                for b, pb in enumerate(positions):
                    table[b, pb // pt] = int(ids[b])
                pages = _poisoned((n_pages, pt, 2, H, 128))
                ops.rope_append_decode_paged(qkv, PagedKV(pages, table.to(DEV)), torch.tensor(positions, dtype=torch.int64, device=DEV),
                                             _inv_freq(), 16.0, q_scale=qs)
                TOTAL["launches"] += 1
                what = f"rope_append_decode_paged B={B} pt={pt} slot {slot} pos {p} prescaled={pre}"
                _same(qkv[slot], want_qkv[0], what + ": q / k left in qkv")
                page = pages[int(ids[slot])]
                _same(page[p % pt], want_row, what + ": the kv row")
                others = torch.ones(pt, dtype=torch.bool, device=DEV)
                others[p % pt] = False
                assert bool((page[others].view(torch.int16) == -1).all()), what + ": another token of the row's page changed"


# ================================================================================================ decode attention at ROWINV_SPLITS
def _subject(p, H):
    """q [1, 1, H, 128] and keys / values [p + 1, 2, H, 128], N(0, 1): one draw per position at H = 32; H = 2 takes its first two heads."""
    if ("subject", p) not in _CACHE:
        _CACHE[("subject", p)] = (_randn(1, 1, 32, 128, seed=7000 + p), _randn(p + 1, 2, 32, 128, seed=8000 + p))
    q, kv = _CACHE[("subject", p)]
    return q[:, :, :H].contiguous(), kv[:, :, :H].contiguous()


def _bank(cap, H):
    """N(0, 1) keys and values for the neighbours that sit at capacity - 1: [>= cap, 2, H, 128], one per H."""
    if ("bank", H) not in _CACHE:
        _CACHE[("bank", H)] = _randn(16384 if H == 32 else 131072, 2, H, 128, seed=9000 + H)
    return _CACHE[("bank", H)][:cap]


def _queries(ops, B, slot, p, H, pre, seed):
    """q [B, 1, H, 128]: the subject's query at `slot` (prescaled as _judge_decode prescales the reference's: on the CPU), N(0, 1) elsewhere."""
    q = _randn(B, 1, H, 128, seed=seed)
    qs = _subject(p, H)[0].cpu()
    q[slot] = ((qs.float() * ops.attn_q_scale(128)).bfloat16() if pre else qs).to(DEV)[0]
    return q


def _attn_reference(ops, p, H, pre):
    """The B = 1 call at capacity p + 1 and 32 splits, held against fp64 op_attention over keys [0, p] inside row 12's pins."""
    if ("ref", p, H, pre) not in _CACHE:
        q, kvs = _subject(p, H)
        kv = _poisoned((2, p + 1, 2, H, 128))
        kv[0] = kvs
        outs, ref, rl2, excess = _judge_decode(q.cpu(), kv, [p], ROWINV_SPLITS, pre)
        TOTAL["launches"] += 2
        print(f"[step rows] decode attention reference p={p} H={H} prescaled={pre}: rel-L2 {rl2:.3e}, worst |err| - bound {excess:+.2e}")
        _assert_decode(outs, ref, rl2, excess, what=f"the one-row reference p={p} H={H} prescaled={pre}")
        _CACHE[("ref", p, H, pre)] = outs[0][0].clone()
    return _CACHE[("ref", p, H, pre)]


def _heads(rows, cap):
    """H = 32 where a cache of `rows` rows stays near 2 GiB, H = 2 otherwise."""
    return 32 if rows * cap * 2 * 32 * 128 * 2 <= 2.5 * GIB else 2


def _neighbours(B, slot, p, cap):
    """(positions, kind per row): the subject at `slot`; the others in turn at position 0, at capacity - 1, and idle (0xFF cache, position 0)."""
    positions, kinds = [], []
    for b in range(B):
        kind = "subject" if b == slot else ("first", "last", "idle")[(b + slot) % 3]
        kinds.append(kind)
        positions.append({"subject": p, "first": 0, "last": cap - 1, "idle": 0}[kind])
    return positions, kinds


def _contiguous_cache(B, slot, p, cap, H):
    _, kvs = _subject(p, H)
    positions, kinds = _neighbours(B, slot, p, cap)
    kv = _poisoned((B, cap, 2, H, 128))
    bank = _bank(cap, H)
    for b, kind in enumerate(kinds):
        if kind == "subject":
            kv[b, :p + 1] = kvs
        elif kind == "first":
            kv[b, 0] = bank[b % cap]
        elif kind == "last":
            kv[b] = bank
    return kv, positions


@pytest.mark.parametrize("p", ATTN_POSITIONS)
def test_decode_attention_row_does_not_see_batch_slot_capacity_or_neighbours(p):
    ops = _ops()
    cases = [(B, cap) for B in ATTN_BS for cap in sorted({p + 1, 4096, 16384}) if cap > p] + [(2, 131072), (9, 131072)]
    for n, (B, cap) in enumerate(cases):
        H = 2 if cap == 131072 else _heads(B, cap)
        for slot in _slots(B):
            kv, positions = _contiguous_cache(B, slot, p, cap, H)
            pos = torch.tensor(positions, dtype=torch.int64, device=DEV)
            for pre in (False, True):
                want = _attn_reference(ops, p, H, pre)
                q = _queries(ops, B, slot, p, H, pre, n + slot)
                out = ops.attention_decode(q, kv[:, :, 0], kv[:, :, 1], pos=pos, n_splits=ROWINV_SPLITS, prescaled=pre)
                TOTAL["launches"] += 1
                _same(out[slot], want, f"decode attention p={p} B={B} slot {slot} capacity {cap} H={H} prescaled={pre}")
            del kv
    torch.cuda.empty_cache()


@pytest.mark.parametrize("p", ATTN_POSITIONS)
def test_paged_decode_attention_row_does_not_see_batch_slot_pages_or_neighbours(p):
    ops = _ops()
    n = 0
    for pt in (64, 128, 256):
        for kind in ("identity", "reversed", "random"):
            B = (2, 9, 33)[n % 3]
            slot = _slots(B)[(n // 3) % len(_slots(B))]
            width = p // pt + 1 + n % 2                                                # the rows at "capacity - 1" fill the last page
            cap = width * pt
            H = _heads(B, cap)
            kv, positions = _contiguous_cache(B, slot, p, cap, H)
            pm = page_map(kind, B, width, seed=p + n, spare=3)
            n_pages = n_pages_of(B, width, 3)
            pages = scatter(kv, pm, pt, n_pages, lengths=[pb + 1 if k != "idle" else 0 for pb, k in zip(positions, _neighbours(B, slot, p, cap)[1])],
                            out=_poisoned((n_pages, pt, 2, H, 128)))
            table = table_of(pm, width + 2)
            for b, (pb, k) in enumerate(zip(positions, _neighbours(B, slot, p, cap)[1])):
                table[b, 0 if k == "idle" else pb // pt + 1:] = 0                       # idle rows and entries behind a row's last page: the scrap page
            rec = PagedKV(pages, table.to(DEV))
            pos = torch.tensor(positions, dtype=torch.int64, device=DEV)
            for pre in (False, True):
                want = _attn_reference(ops, p, H, pre)
                q = _queries(ops, B, slot, p, H, pre, n + 50)
                out = ops.attention_decode_paged(q, rec, pos, n_splits=ROWINV_SPLITS, prescaled=pre)
                TOTAL["launches"] += 1
                _same(out[slot], want, f"paged decode attention p={p} B={B} slot {slot} pt={pt} {kind} map, width {width}, H={H} prescaled={pre}")
            del kv, pages
            n += 1
    torch.cuda.empty_cache()


def test_zz_totals():
    """The module's totals (tests/PARITY_batch_invariant.md section 3 is filled from this line)."""
    dt = time.time() - TOTAL["t0"] if TOTAL["t0"] else 0.0
    print(f"[step rows total] launches {TOTAL['launches']}, elements compared {TOTAL['elements']}, mismatching {TOTAL['mismatches']}; "
          f"wall time since the first test {dt:.1f} s")
    assert TOTAL["mismatches"] == 0
