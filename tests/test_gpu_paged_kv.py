"""GPU (-m gpu): the paged KV cache of the decode pool (csrc/kv_paged.hip; DESIGN.md section 23, tests/PARITY_paged_kv.md).

  * evo_attn_decode_paged_bf16 against its contiguous sibling, BITWISE: exact key sets (tests/attn_exact.py, designs U / D / D' / S)
    scattered into pages under four page maps; for the same keys, positions and n_splits the output must be torch.equal to
    evo_attn_decode_bf16's, and inside attn_exact.judge's rule against the fp64 expectation.  Every page slot no row owns, every token
    behind a row's position inside its last page and the whole scrap page 0 hold 0xFF (NaN): none of it may reach an output.  Two
    launches must agree bit for bit;
  * one case whose live pages lie beyond 4 GiB from the pool's base (the page base is 64-bit);
  * evo_rope_append_decode_paged_bf16 against evo_rope_append_decode_bf16: the q and k left in qkv, the row written, and -- by canaries --
    that no other byte of the pool changed; write path -> read path over 3 page_tokens + 1 steps, step for step;
  * both entries inside the poisoned arena (tests/arena.py) at 16-byte alignment;
  * DecodePool(kv_paged=True) on the toy model against the unpaged pool: ids and recorded logits torch.equal, in shapes where both
    derive the same n_splits."""
import math

import pytest
import torch

import attn_exact as X
from evo_amd.sh.cache import PagedKV
from paged_ref import PAGE_MAPS, n_pages_of, page_map, scatter, table_of
from test_gpu_arena import _run, covers, gen, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
SPLITS = [1, 4, 8, 40, None]


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


def _dims(n):
    return (X.DIMS2 + X.DIMS3)[n % 5]


def _contiguous(ops, q, kv, positions, n_splits, pre):
    """evo_attn_decode_bf16 on kv [B, cap, 2, H, 128] with per-row positions."""
    from evo_amd.ops import _check, _stream
    B, _, H, hd = q.shape
    k, v = kv[:, :, 0], kv[:, :, 1]
    pos = torch.tensor(positions, dtype=torch.int64, device=DEV)
    o = _poisoned((B, 1, H, hd))
    part_o, part_ml = _poisoned((B, H, n_splits, hd), torch.float32), _poisoned((B, H, n_splits, 2), torch.float32)
    _check(ops.lib.evo_attn_decode_bf16(q.data_ptr(), k.data_ptr(), v.data_ptr(), o.data_ptr(), B, H, k.shape[1], q.stride(0), q.stride(2),
                                        k.stride(0), k.stride(1), k.stride(2), v.stride(0), v.stride(1), v.stride(2), pos.data_ptr(),
                                        part_o.data_ptr(), part_ml.data_ptr(), n_splits, 0.0 if pre else 1.0 / math.sqrt(hd), _stream()),
           "evo_attn_decode_bf16")
    return o


def _paged(ops, q, pages, table, positions, n_splits, pre):
    """The C entry as HipOps.attention_decode_paged calls it, caller-owned part_o / part_ml pre-filled with NaN; two launches, all three
    outputs bit-identical."""
    from evo_amd.ops import _check, _stream
    B, _, H, hd = q.shape
    pos = torch.tensor(positions, dtype=torch.int64, device=DEV)
    outs = []
    for _ in range(2):
        o = _poisoned((B, 1, H, hd))
        part_o, part_ml = _poisoned((B, H, n_splits, hd), torch.float32), _poisoned((B, H, n_splits, 2), torch.float32)
        _check(ops.lib.evo_attn_decode_paged_bf16(q.data_ptr(), pages.data_ptr(), table.data_ptr(), o.data_ptr(), B, H, pages.shape[1],
                                                  pages.shape[0], table.shape[1], q.stride(0), q.stride(2), pages.stride(0), pages.stride(1),
                                                  pages.stride(2), pages.stride(3), pos.data_ptr(), part_o.data_ptr(), part_ml.data_ptr(),
                                                  n_splits, 0.0 if pre else 1.0 / math.sqrt(hd), _stream()), "evo_attn_decode_paged_bf16")
        outs.append((o, part_o, part_ml))
    torch.cuda.synchronize()
    for a, b in zip(*outs):
        assert torch.equal(_bits(a), _bits(b)), "two launches differ"
    return outs[0][0]


def _case(ops, design, positions, H, pt, kind, ns, pre, seed, what, extra_width=2, spare=3):
    """One exact case, paged against contiguous.  The pool is 0xFF except tokens [0, positions[b]] of every row's pages."""
    B = len(positions)
    width = max(positions) // pt + 1
    n_splits = ops._decode_splits((width + extra_width) * pt) if ns is None else ns      # HipOps.attention_decode_paged's default
    c = X.build_decode(design, positions, H, _dims(seed), n_splits, DEV)
    kvc = torch.stack([c["k"], c["v"]], 2)                            # [B, Tk, 2, H, 128]
    cap = kvc.shape[1] + 37
    kv = _poisoned((B + 1, cap, 2, H, 128))
    for b, p in enumerate(positions):
        kv[b, :p + 1] = kvc[b, :p + 1]
    pm = page_map(kind, B, width, seed=seed, spare=spare)
    n_pages = n_pages_of(B, width, spare)
    pages = scatter(kvc, pm, pt, n_pages, lengths=[p + 1 for p in positions], out=_poisoned((n_pages, pt, 2, H, 128)))
    # entries behind a row's last page hold 0 -- also inside the needed width, for the shorter rows -- and the table is wider than any row needs
    table = table_of(pm, width + extra_width)
    for b, p in enumerate(positions):
        table[b, p // pt + 1:] = 0
    table = table.to(DEV)
    want = _contiguous(ops, c["q"], kv[:B], positions, n_splits, pre)
    got = _paged(ops, c["q"], pages, table, positions, n_splits, pre)
    assert torch.equal(_bits(got), _bits(want)), f"{what}: paged differs from evo_attn_decode_bf16 in rows " \
                                                 f"{(_bits(got) != _bits(want)).flatten(1).any(1).nonzero().flatten().tolist()}"
    ref, single = X.expected(c["lev"], c["v"], c["mult"])
    ver = X.judge(got, ref, single)
    assert ver.ok, f"{what}: {ver}; first bad rows (b, query) {ver.bad.nonzero()[:8].tolist()}"


def test_every_key_count_up_to_seven_pages(ops):
    """n_keys = 1 .. 448 at page_tokens = 64, eight rows of unequal length per launch, H = 1: every ragged half, every block and page seam.
    U counts the keys a row saw, D returns the row's last key; the map and the split count rotate."""
    n = 0
    for p0 in range(0, 448, 8):
        positions = list(range(p0, p0 + 8))
        for design in ("U", "D"):
            kind, ns = PAGE_MAPS[n % 4], SPLITS[n % 5]
            _case(ops, design, positions, 1, 64, kind, ns, bool(n & 1), n, f"n_keys {p0 + 1}..{p0 + 8} {design} {kind} splits {ns}")
            n += 1


@pytest.mark.parametrize("ns", SPLITS, ids=[f"splits{ns}" for ns in SPLITS])
@pytest.mark.parametrize("pt", [64, 128, 256])
def test_decode_positions_on_exact_key_sets(ops, pt, ns):
    """attn_exact.DECODE_POSITIONS (around every half and block, two long rows) mixed in one batch of twelve; four designs, both score
    forms, the four page maps in turn."""
    for i, design in enumerate(X.DESIGNS):
        for pre in (False, True):
            kind = PAGE_MAPS[(i + 2 * pre + pt // 64) % 4]
            _case(ops, design, X.DECODE_POSITIONS, 2, pt, kind, ns, pre, i + (0 if ns is None else ns),
                  f"positions {design} {'PRE' if pre else 'plain'} pt {pt} {kind} splits {ns}")


@pytest.mark.parametrize("kind", PAGE_MAPS)
@pytest.mark.parametrize("H", [1, 32])
@pytest.mark.parametrize("positions", [[447], [5, 200, 447], [0, 31, 32, 63, 64, 130, 300, 383]], ids=["B1", "B3", "B8"])
def test_batches_heads_and_maps(ops, positions, H, kind):
    for i, (design, pt, ns) in enumerate((("U", 64, None), ("D", 128, 4), ("S", 64, 8), ("D'", 256, 40), ("S", 256, 1))):
        _case(ops, design, positions, H, pt, kind, ns, bool(i & 1), i + H, f"B {len(positions)} H {H} {design} pt {pt} {kind} splits {ns}")


def test_live_pages_beyond_four_gib_of_the_pool(ops):
    """H = 1, page_tokens = 64: a page is 32 KiB, so page ids >= 131,072 lie beyond 4 GiB from the pool's base.  The pool is allocated and
    never filled; only its last pages are written and read."""
    H, pt, positions = 1, 64, [100, 191]
    n_pages = 131072 + 8
    try:
        pages = torch.empty(n_pages, pt, 2, H, 128, dtype=BF, device=DEV)
    except RuntimeError as e:                                          # (torch.cuda.OutOfMemoryError is one)
        pytest.skip(f"no room for a {n_pages * pt * 2 * H * 256 / 2 ** 30:.2f} GiB page pool: {e}")
    assert pages.stride(0) * 2 * 131072 == 1 << 32
    ids = torch.tensor([[n_pages - 1, n_pages - 3, n_pages - 5], [n_pages - 6, n_pages - 2, n_pages - 4]])
    assert int(ids.min()) >= 131072
    pages[n_pages - 8:].view(-1).view(torch.uint8).fill_(0xFF)
    for i, (design, ns) in enumerate((("U", 4), ("D", None), ("S", 8))):
        n_splits = ops._decode_splits(3 * pt) if ns is None else ns
        c = X.build_decode(design, positions, H, _dims(i), n_splits, DEV)
        kvc = torch.stack([c["k"], c["v"]], 2)
        kv = _poisoned((3, kvc.shape[1] + 37, 2, H, 128))
        for b, p in enumerate(positions):
            kv[b, :p + 1] = kvc[b, :p + 1]
        scatter(kvc, ids, pt, n_pages, lengths=[p + 1 for p in positions], out=pages)
        table = table_of(ids).to(DEV)
        want = _contiguous(ops, c["q"], kv[:2], positions, n_splits, False)
        got = _paged(ops, c["q"], pages, table, positions, n_splits, False)
        assert torch.equal(_bits(got), _bits(want)), design
        assert X.judge(got, *X.expected(c["lev"], c["v"], c["mult"])).ok, design
    del pages
    torch.cuda.empty_cache()


# ================================================================================================ the append
def _inv_freq(hd=128):
    return (1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32, device=DEV) / hd))).contiguous()


@pytest.mark.parametrize("q_scale", [1.0, None])
@pytest.mark.parametrize("pt,H", [(64, 2), (256, 32), (128, 3)])
def test_append_equals_the_contiguous_append_and_touches_one_row(ops, pt, H, q_scale):
    """Positions 0, page_tokens - 1, page_tokens, the last row of the last table entry, two in between; an idle row (table row 0, pos 0)
    writes the scrap page only.  Every other byte of the pool keeps its 0xFF."""
    width = 3
    positions = [0, pt - 1, pt, width * pt - 1, pt + 17, 2 * pt + 5, 0]
    B = len(positions)
    idle = B - 1
    qs = ops.attn_q_scale(128) if q_scale is None else q_scale
    pm = page_map("random", B, width, seed=pt + H, spare=2)
    n_pages = n_pages_of(B, width, 2)
    table = table_of(pm, width + 1)
    table[idle] = 0
    pos = torch.tensor(positions, dtype=torch.int64, device=DEV)
    qkv = rnd((B, 1, 3, H, 128), gen(pt + H))
    qkv_c, qkv_p = qkv.clone(), qkv.clone()
    kv = _poisoned((B, width * pt, 2, H, 128))
    ops.rope_append_decode(qkv_c, kv, pos, _inv_freq(), 16.0, q_scale=qs)
    pages = _poisoned((n_pages, pt, 2, H, 128))
    rec = PagedKV(pages, table.to(DEV))
    ops.rope_append_decode_paged(qkv_p, rec, pos, _inv_freq(), 16.0, q_scale=qs)
    torch.cuda.synchronize()
    assert torch.equal(_bits(qkv_p), _bits(qkv_c)), "q / k left in qkv differ from rope_append_decode's"
    want = _poisoned((n_pages, pt, 2, H, 128))
    for b, p in enumerate(positions):
        want[int(table[b, p // pt]), p % pt] = kv[b, p]
    assert int(table[idle, 0]) == 0 and not torch.equal(_bits(want[0, 0]), _bits(_poisoned((2, H, 128))))     # the idle row landed in page 0
    assert torch.equal(pages.view(-1).view(torch.uint8), want.view(-1).view(torch.uint8)), "a byte outside the appended rows changed"


def test_write_path_then_read_path_step_for_step(ops):
    """3 page_tokens + 1 steps of append + attention, paged and contiguous side by side from the same qkv: every step's output and every
    qkv left behind torch.equal."""
    pt, H, B, width = 64, 2, 3, 4
    steps = 3 * pt + 1
    pm = page_map("random", B, width, seed=7, spare=2)
    pages = _poisoned((n_pages_of(B, width, 2), pt, 2, H, 128))
    rec = PagedKV(pages, table_of(pm, width).to(DEV))
    kv = _poisoned((B, width * pt, 2, H, 128))
    src = rnd((steps, B, 1, 3, H, 128), gen(3))
    pos = torch.zeros(B, dtype=torch.int64, device=DEV)
    n_splits = ops._decode_splits(width * pt)
    assert n_splits == ops._decode_splits(kv.shape[1])                # both sides derive the same split count
    got, want = [], []
    for s in range(steps):
        a, b = src[s].clone(), src[s].clone()
        ops.rope_append_decode(a, kv, pos, _inv_freq(), 1.0)
        ops.rope_append_decode_paged(b, rec, pos, _inv_freq(), 1.0)
        want.append((a, ops.attention_decode(a[:, :, 0], kv[:, :, 0], kv[:, :, 1], pos=pos)))
        got.append((b, ops.attention_decode_paged(b[:, :, 0], rec, pos)))
        pos += 1
    torch.cuda.synchronize()
    for s in range(steps):
        assert torch.equal(_bits(got[s][0]), _bits(want[s][0])) and torch.equal(_bits(got[s][1]), _bits(want[s][1])), f"step {s}"
    assert bool(torch.isfinite(want[-1][1].float()).all())


# ================================================================================================ the arena
@covers("evo_rope_append_decode_paged_bf16")
@pytest.mark.parametrize("q_scale", [1.0, None])
def test_arena_append(q_scale):
    from test_gpu_arena import _ops
    ops, pt, H, width = _ops(), 64, 2, 2
    positions = [0, pt - 1, pt, 2 * pt - 1, 70]
    B = len(positions)
    pm = page_map("reversed", B, width)
    inp = {"qkv": rnd((B, 1, 3, H, 128), gen(9)), "pages": rnd((n_pages_of(B, width), pt, 2, H, 128), gen(1)), "table": table_of(pm, width).to(DEV),
           "pos": torch.tensor(positions, dtype=torch.int64, device=DEV), "inv": _inv_freq()}
    qs = ops.attn_q_scale(128) if q_scale is None else q_scale
    _run(lambda qkv, pages, table, pos, inv: ops.rope_append_decode_paged(qkv, PagedKV(pages, table), pos, inv, 16.0, q_scale=qs), inp,
         inout=["qkv", "pages"], expect=["evo_rope_append_decode_paged_bf16"], align={"pos": 8, "table": 4})


@covers("evo_attn_decode_paged_bf16")
@pytest.mark.parametrize("B,H,pt,n_keys,splits", [(2, 2, 64, 1, None), (1, 2, 64, 65, 3), (2, 3, 128, 2048 + 33, None), (2, 3, 256, 2048 + 33, 5),
                                                  (3, 2, 64, 448, None)])
def test_arena_attention(B, H, pt, n_keys, splits):
    """The pool, the table, pos, part_o / part_ml are carved; the last row sits at n_keys - 1, the last token of a partly used page."""
    from test_gpu_arena import _ops
    ops, width = _ops(), -(-n_keys // pt)
    pm = page_map("interleaved", B, width)
    inp = {"q": rnd((B, 1, H, 128), gen(n_keys)), "pages": rnd((n_pages_of(B, width), pt, 2, H, 128), gen(2)),
           "table": table_of(pm, width + 1).to(DEV),
           "pos": torch.tensor([max(0, n_keys - 1 - 40 * (B - 1 - b)) for b in range(B)], dtype=torch.int64, device=DEV)}
    _run(lambda q, pages, table, pos: ops.attention_decode_paged(q, PagedKV(pages, table), pos, n_splits=splits), inp,
         expect=["evo_attn_decode_paged_bf16"], align={"pos": 8, "table": 4})


# ================================================================================================ model / pool on the toy model
from test_gpu_pool import PROMPTS  # noqa: E402

N_TOK = 8
# Both pools derive n_splits from the slot's bound: the unpaged pool from its capacity (longest prompt + the largest limit on a pool's first
# call), the paged pool from table_width * page_tokens.  _decode_splits saturates at 32 from 1,793 keys on, so with the long prompt in the
# set (capacity 2,216 unpaged; 9 x 256 = 2,304 and 35 x 64 = 2,240 paged) all of them derive 32; _same_splits asserts it in every test.
LONG4 = "ACGTTGCAAGGCTTAACCGGATAT" * 92                               # 2,208 nt: 9 pages of 256 with its tokens, 35 of 64


def _build_toy(weight_fp8=False):
    from test_gpu_model import SMALL4, build
    cfgd = dict(SMALL4, use_interpolated_rotary_pos_emb=True, rotary_emb_scaling_factor=16)
    return build(cfgd)[2]


def _pool(m, n_slots, **kw):
    from evo_amd.pool import DecodePool
    from evo_amd.tokenizer import CharLevelTokenizer
    return DecodePool(m, CharLevelTokenizer(512), n_slots=n_slots, top_k=4, top_p=1.0, temperature=0.7, device=DEV, **kw)


@pytest.fixture(scope="module")
def toy():
    return _build_toy()


def _same_splits(ops, unpaged, paged):
    a, b = ops._decode_splits(unpaged.capacity), ops._decode_splits(paged.table.shape[1] * paged.page_tokens)
    assert a == b, (a, b, unpaged.capacity, paged.table.shape)


MIXED = [LONG4] + PROMPTS                                             # one prompt of many pages among short ones


@pytest.mark.parametrize("n_slots,use_graph,prefill_batch,pt", [(3, False, 1, 256), (8, True, 1, 256), (3, True, 4, 64), (8, False, 4, 256)])
def test_paged_pool_equals_the_unpaged_pool(toy, n_slots, use_graph, prefill_batch, pt):
    """Seeded device sampler, so both pools draw the same tokens as long as their logits agree bit for bit -- which they must: the step's
    other launches are the same, and the two attention launches are bitwise the siblings' at the same n_splits."""
    kw = dict(use_graph=use_graph, seed=5, prefill_batch=prefill_batch)
    ref = _pool(toy, n_slots, **kw)
    want = ref.generate(MIXED, n_tokens=N_TOK, n_sample_per_prompt=2)
    pool = _pool(toy, n_slots, kv_paged=True, kv_page_tokens=pt, **kw)
    got = pool.generate(MIXED, n_tokens=N_TOK, n_sample_per_prompt=2)
    _same_splits(toy.ops, ref, pool)
    assert torch.equal(pool.last_ids, ref.last_ids) and torch.equal(pool.last_logits, ref.last_logits) and got == want
    assert pool.stats["kv_bytes"] < ref.stats["kv_bytes"], (pool.stats["kv_bytes"], ref.stats["kv_bytes"])
    needs = [-(-(len(p) + N_TOK) // pt) for p in MIXED for _ in range(2)]
    assert pool.stats["kv_pages"] == 1 + sum(sorted(needs, reverse=True)[:n_slots])
    # equal limits: jobs run in waves of n_slots consecutive jobs
    assert pool.stats["kv_pages_peak"] == max(sum(needs[j:j + n_slots]) for j in range(0, len(needs), n_slots))
    assert sorted(pool._free_pages) == list(range(1, pool.stats["kv_pages"])) and not bool(pool.table.any())


def test_mixed_lengths_under_a_budget_with_stop_rules_and_a_constraint(toy):
    """The job-control path: per-prompt limits, a stop sequence, one constrained prompt; a budget well below n_slots x the longest job, so
    the short jobs wait for pages the long one holds, pages are freed and reused, and everything still equals the unpaged pool."""
    import evo_amd
    pt, n_slots = 64, 4
    limits = [12] + [20, 6, 9, 30, 6, 14]
    cons = [None, evo_amd.iupac_template("ATGNNRYNTAA"), None, None, None, None, None]
    gen_kw = dict(n_tokens=limits, n_sample_per_prompt=2, stop_sequences=["TAA", "GG"], stop_frame=3, constraints=cons)
    kw = dict(use_graph=True, seed=9, allowed_tokens="ACGT")
    ref = _pool(toy, n_slots, **kw)
    want = ref.generate(MIXED, **gen_kw)
    needs = [-(-(len(p) + l) // pt) for p, l in zip(MIXED, limits)]
    budget = (max(needs) + 4) * pt                                    # the long job plus four pages; n_slots x longest would be 4 x 35 pages
    assert budget < n_slots * max(needs) * pt // 3
    pool = _pool(toy, n_slots, kv_paged=True, kv_page_tokens=pt, kv_budget_tokens=budget, **kw)
    got = pool.generate(MIXED, **gen_kw)
    _same_splits(toy.ops, ref, pool)
    assert got == want and torch.equal(pool.last_ids, ref.last_ids) and torch.equal(pool.last_logits, ref.last_logits)
    assert pool.last_lengths == ref.last_lengths and pool.last_finish == ref.last_finish
    assert pool.stats["kv_page_waits"] > 0 and pool.stats["kv_pages"] == 1 + max(needs) + 4
    assert pool.stats["kv_bytes"] * 3 < ref.stats["kv_bytes"]
    assert sorted(pool._free_pages) == list(range(1, pool.stats["kv_pages"])) and not bool(pool.table.any())


def test_fp8_weights_compose(toy):
    kw = dict(use_graph=True, seed=2, weight_dtype="fp8")
    ref = _pool(toy, 4, **kw)
    want = ref.generate(MIXED[:4], n_tokens=N_TOK, n_sample_per_prompt=2)
    pool = _pool(toy, 4, kv_paged=True, kv_page_tokens=256, **kw)
    got = pool.generate(MIXED[:4], n_tokens=N_TOK, n_sample_per_prompt=2)
    _same_splits(toy.ops, ref, pool)
    assert got == want and torch.equal(pool.last_ids, ref.last_ids) and torch.equal(pool.last_logits, ref.last_logits)
    assert pool.stats["weight_dtype"] == "fp8" and pool.stats["kv_bytes"] < ref.stats["kv_bytes"]
