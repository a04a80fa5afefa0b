"""CPU: the opt-in paged KV cache of the decode pool -- the layers that need no GPU.

  * the two C entries: exported, declared, bound, ABI still 20, every contract violation refused with -1 before any launch (the pointers
    passed are never dereferenced);
  * the allocator: page 0 is never handed out, exhaustion makes admission wait, an oversized job is refused before any forward, every
    page and every table row is back after generate() -- stop-rule and constraint endings included;
  * the scheduler and the model plumbing on the fp64 oracle backend (tests/paged_ref.PagedOps: gather + the contiguous oracle op): the
    paged pool equals the unpaged pool in ids and logits by torch.equal -- the gather hands the oracle the very keys the contiguous
    cache holds, in the same order;
  * the refused combinations;
  * resources: the two kernels without scratch, the attention without LDS, inside two waves per SIMD and the sibling's registers + 8."""
import ctypes
import os
import re

import pytest
import torch

from evo_amd import _build
from evo_amd import constraints as K
from evo_amd import ops as evo_ops
from evo_amd.backend import Backend
from evo_amd.pool import DecodePool, sample_many
from evo_amd.sh.cache import InferenceParams, PagedKV, PromptStore, SharedPrefix
from paged_ref import PagedOps, PagedOracleOps, gather, n_pages_of, page_map, scatter, table_of
from test_constraints_host import DfaOracleOps
from test_gpu_pool import PROMPTS
from test_kernel_resources import HIPCC, _metadata
from test_ragged_prefill_host import SMALL, TOK, RaggedOracleOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("evo_rope_append_decode_paged_bf16", "evo_attn_decode_paged_bf16")


# ------------------------------------------------------------------------------------------------ C ABI
def test_entries_are_wired():
    header = open(os.path.join(ROOT, "include", "evo_mi355x.h")).read()
    for name in ENTRIES:
        assert name in _build.EXPORTS and name in evo_ops._SIGNATURES and re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert int(re.search(r"#define EVO_ABI_VERSION (\d+)", header).group(1)) == evo_ops.ABI_VERSION == 20     # additive: no signature changed
    assert evo_ops.load_library().evo_abi_version() == 20
    assert Backend.OPTIONAL["kv_paged"] == ("rope_append_decode_paged", "attention_decode_paged")
    for meth in Backend.OPTIONAL["kv_paged"]:
        assert hasattr(evo_ops.HipOps, meth), meth
    assert any(p.name == "kv_paged.hip" for p in _build.sources())
    assert InferenceParams(max_seqlen=8, max_batch_size=1).kv_layout == "contiguous"
    text = open(os.path.join(ROOT, "scripts", "sample_many.py")).read()
    for flag in ("--kv-paged", "--kv-page-tokens", "--kv-budget-tokens"):
        assert flag in text, flag
    import inspect
    for fn in (DecodePool.__init__, sample_many):
        assert {"kv_paged", "kv_page_tokens", "kv_budget_tokens"} <= set(inspect.signature(fn).parameters)


ONE = ctypes.c_void_p(16)                                             # non-null, 16-byte aligned, never dereferenced
F = ctypes.c_float
# H = 2: a page of 64 tokens is [64, 2, 2, 128]
CACHE_OK = dict(page_tokens=64, n_pages=5, table_width=3, p_sp=64 * 512, p_st=512, p_sw=256, p_sh=128)
CACHE_NAMES = list(CACHE_OK)
CACHE_BAD = [dict(page_tokens=0), dict(page_tokens=32), dict(page_tokens=96), dict(page_tokens=192), dict(page_tokens=-64), dict(n_pages=0),
             dict(table_width=0), dict(n_pages=1 << 31), dict(table_width=1 << 31), dict(p_sp=64 * 512 + 4), dict(p_st=516), dict(p_sw=260),
             dict(p_sh=132), dict(p_st=64), dict(p_sw=0), dict(p_sh=0), dict(p_sp=-8),
             # a page's span in bytes (page_tokens * p_st * 2) must stay below 2^32 - 1: the lane's offset inside a page is 32-bit
             dict(page_tokens=1 << 20, p_st=2048), dict(page_tokens=64, p_st=1 << 25), dict(page_tokens=1 << 31, p_st=512)]


def _caller(name, names, ok):
    f = getattr(evo_ops.load_library(), name)
    assert list(ok) == names and len(evo_ops._SIGNATURES[name][0]) == len(names)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return f(*[a[n] for n in names])
    return call


def test_rope_append_paged_refuses_before_any_launch():
    names = ["qkv", "pages", "table", "pos", "inv_freq", "scaling", "B", "H", "hd"] + CACHE_NAMES + ["q_scale", "stream"]
    ok = dict(qkv=ONE, pages=ONE, table=ONE, pos=ONE, inv_freq=ONE, scaling=F(1.0), B=2, H=2, hd=128, **CACHE_OK, q_scale=F(1.0), stream=None)
    call = _caller("evo_rope_append_decode_paged_bf16", names, ok)
    for n in ("qkv", "pages", "table", "pos", "inv_freq"):
        assert call(**{n: None}) == -1, n
    for n in ("qkv", "pages"):
        assert call(**{n: ctypes.c_void_p(8)}) == -1 and call(**{n: ctypes.c_void_p(24)}) == -1, n
    assert call(pos=ctypes.c_void_p(20)) == -1 and call(inv_freq=ctypes.c_void_p(18)) == -1 and call(table=ctypes.c_void_p(18)) == -1
    for kw in (dict(B=0), dict(H=0), dict(hd=64), dict(hd=256), dict(hd=0), dict(scaling=F(0.0)), dict(scaling=F(-1.0)), dict(q_scale=F(0.0)),
               dict(q_scale=F(float("nan"))), dict(scaling=F(float("nan")))):
        assert call(**kw) == -1, kw
    for kw in CACHE_BAD:
        assert call(**kw) == -1, kw


def test_attn_decode_paged_refuses_before_any_launch():
    names = ["q", "pages", "table", "o", "B", "H"] + CACHE_NAMES[:3] + ["q_sb", "q_sh"] + CACHE_NAMES[3:] + ["pos", "part_o", "part_ml", "n_splits",
                                                                                                        "softmax_scale", "stream"]
    ok = dict(q=ONE, pages=ONE, table=ONE, o=ONE, B=2, H=2, **{n: CACHE_OK[n] for n in CACHE_NAMES[:3]}, q_sb=768, q_sh=128,
              **{n: CACHE_OK[n] for n in CACHE_NAMES[3:]}, pos=ONE, part_o=ONE, part_ml=ONE, n_splits=4, softmax_scale=F(0.0), stream=None)
    call = _caller("evo_attn_decode_paged_bf16", names, ok)
    for n in ("q", "pages", "table", "o", "pos", "part_o", "part_ml"):          # pos is required
        assert call(**{n: None}) == -1, n
    for n in ("q", "pages", "o", "part_o"):
        assert call(**{n: ctypes.c_void_p(8)}) == -1, n
    assert call(pos=ctypes.c_void_p(20)) == -1 and call(table=ctypes.c_void_p(18)) == -1 and call(part_ml=ctypes.c_void_p(18)) == -1
    for kw in (dict(B=0), dict(H=0), dict(n_splits=0), dict(n_splits=-1), dict(n_splits=1025), dict(H=65536), dict(B=65536), dict(q_sb=772),
               dict(q_sh=132)):
        assert call(**kw) == -1, kw
    for kw in CACHE_BAD:
        assert call(**kw) == -1, kw


# ------------------------------------------------------------------------------------------------ the helper
@pytest.mark.parametrize("kind", ["identity", "reversed", "interleaved", "random"])
def test_page_maps_scatter_and_gather(kind):
    B, width, pt, spare = 3, 4, 64, 5
    pm = page_map(kind, B, width, seed=2, spare=spare)
    ids = pm.reshape(-1).tolist()
    assert len(set(ids)) == B * width and min(ids) >= 1 and max(ids) < n_pages_of(B, width, spare)      # distinct, never the scrap page
    cache = torch.randn(B, width * pt - 7, 2, 2, 128)
    pages = scatter(cache, pm, pt, n_pages_of(B, width, spare))
    assert torch.equal(gather(pages, table_of(pm, width + 2), cache.shape[1]), cache)
    owned = torch.zeros(pages.shape[0], dtype=torch.bool)
    owned[pm.reshape(-1)] = True
    assert not bool(pages[~owned].any()) and int((~owned).sum()) == 1 + spare
    if kind != "identity":
        assert pm.reshape(-1).tolist() != sorted(ids)


# ------------------------------------------------------------------------------------------------ the backend
class PagedCtlOps(PagedOps, DfaOracleOps, RaggedOracleOps):
    """The oracle backend with the sampler launches of the job-control path and the group "kv_paged"."""

    def __init__(self, act=torch.float64):
        super().__init__(act)
        self.paged_calls = {"append": 0, "decode": 0}


def _model(ops):
    from oracle.stripedhyena_ref import RefConfig, make_synthetic_state_dict
    from evo_amd.sh.model import StripedHyena
    sd = make_synthetic_state_dict(RefConfig.from_dict(SMALL), seed=3)
    m = StripedHyena(dict(SMALL), ops=ops)
    m.load_state_dict({k: (v.double() if v.dtype == torch.bfloat16 else v) for k, v in sd.items()})
    return m


@pytest.fixture(scope="module")
def small():
    return _model(PagedCtlOps(torch.float64))


N_TOK, N_SPP = 6, 2
LENS = [len(p) for p in PROMPTS]                                      # 81, 8, 145, 1, 69, 160: with 6 tokens 2, 1, 3, 1, 2, 3 pages of 64


def _need(n_keys, pt):
    return -(-n_keys // pt)


def _assert_all_pages_back(pool):
    assert sorted(pool._free_pages) == list(range(1, pool.stats["kv_pages"])), "a page is missing from (or twice on) the free list"
    assert 0 not in pool._free_pages and not any(pool._slot_pages)
    assert not bool(pool.table.any()), "a table row still names a page"
    for kv in pool.ipd["mha"].key_value_memory_dict.values():
        assert isinstance(kv, PagedKV) and kv.table is pool.table


def _greedy(m, n_slots, prefill_batch=1, **kw):
    pool = DecodePool(m, TOK, n_slots=n_slots, top_k=1, top_p=1.0, temperature=0.0, device="cpu", prefill_batch=prefill_batch, **kw)
    out = pool.generate(PROMPTS, n_tokens=N_TOK, n_sample_per_prompt=N_SPP)
    return (pool,) + tuple(out)


_UNPAGED = {}


def unpaged(m, n_slots, prefill_batch):
    """The yardstick, computed once per shape: the pool as it is without the option."""
    key = (n_slots, prefill_batch)
    if key not in _UNPAGED:
        pool, seqs, scores, owner = _greedy(m, n_slots, prefill_batch)
        _UNPAGED[key] = (pool.last_ids.clone(), pool.last_logits.clone(), seqs, scores, owner, dict(pool.stats))
    return _UNPAGED[key]


@pytest.mark.parametrize("page_tokens", [64, 128])
@pytest.mark.parametrize("prefill_batch", [1, 4])
@pytest.mark.parametrize("n_slots", [1, 3, 4])
def test_paged_pool_equals_the_unpaged_pool(small, n_slots, prefill_batch, page_tokens):
    ids, logits, seqs, scores, owner, stats = unpaged(small, n_slots, prefill_batch)
    small.ops.paged_calls = {"append": 0, "decode": 0}
    pool, seqs_p, scores_p, owner_p = _greedy(small, n_slots, prefill_batch, kv_paged=True, kv_page_tokens=page_tokens)
    assert torch.equal(pool.last_ids, ids) and torch.equal(pool.last_logits, logits)
    assert (seqs_p, scores_p, owner_p) == (seqs, scores, owner)
    assert pool.stats["steps"] == stats["steps"] and pool.stats["prefills"] == stats["prefills"] and pool.stats["kv_page_waits"] == 0
    assert small.ops.paged_calls["append"] == small.ops.paged_calls["decode"] == pool.stats["steps"] > 0      # one attention layer
    needs = [_need(n + N_TOK, page_tokens) for n in LENS for _ in range(N_SPP)]
    if page_tokens == 64:
        assert set(needs) == {1, 2, 3}                               # jobs of one, two and three pages
    # sized for the n_slots largest needs (+ the scrap page); the table is as wide as the largest
    assert pool.stats["kv_pages"] == 1 + sum(sorted(needs, reverse=True)[:n_slots]) and pool.table.shape == (n_slots, max(needs))
    assert pool.ipd["mha"].kv_layout == "paged" and pool.capacity == max(needs) * page_tokens
    H, hd, L = small.num_heads, small.head_dim, len(small.attn_layer_idxs)
    assert pool.stats["kv_bytes"] == pool.stats["kv_pages"] * page_tokens * 2 * H * hd * 8 * L           # (an fp64 oracle model: 8-byte elements)
    # jobs are admitted in order and equal-length jobs end together: the peak is the best window of n_slots consecutive jobs
    assert pool.stats["kv_pages_peak"] == max(sum(needs[j:j + n_slots]) for j in range(0, len(needs), n_slots))
    _assert_all_pages_back(pool)


def test_pages_are_reused_out_of_order_and_page_zero_is_never_handed_out(small, monkeypatch):
    """Slots are re-filled with pages freed by earlier jobs: the maps a job gets are no longer monotonic, and the outputs do not care."""
    seen = []
    orig = DecodePool._install

    def spy(self, slot, tmp, P, row=0, need=0):
        orig(self, slot, tmp, P, row=row, need=need)
        seen.append(list(self._slot_pages[slot]))
        assert self.table[slot, :need].tolist() == seen[-1] and not bool(self.table[slot, need:].any())
    monkeypatch.setattr(DecodePool, "_install", spy)
    ids, logits = unpaged(small, 3, 1)[:2]
    pool = _greedy(small, 3, 1, kv_paged=True, kv_page_tokens=64)[0]
    assert torch.equal(pool.last_ids, ids) and torch.equal(pool.last_logits, logits)
    assert len(seen) == len(PROMPTS) * N_SPP and all(0 not in pg and len(set(pg)) == len(pg) for pg in seen)
    assert any(pg != sorted(pg) for pg in seen), "no job ever got a non-monotonic page list"
    assert [len(pg) for pg in seen] == [_need(n + N_TOK, 64) for n in LENS for _ in range(N_SPP)]
    # a second call on the same pool: nothing grows, nothing is copied, the free list is whole again
    pages0 = {i: kv.pages for i, kv in pool.ipd["mha"].key_value_memory_dict.items()}
    pool.generate(PROMPTS[:2], n_tokens=N_TOK, n_sample_per_prompt=1)
    assert all(pool.ipd["mha"].key_value_memory_dict[i].pages is p for i, p in pages0.items())
    assert torch.equal(pool.last_ids, ids[[0, 2]]) and torch.equal(pool.last_logits, logits[[0, 2]])
    _assert_all_pages_back(pool)


def test_a_tight_budget_waits_in_order_and_changes_nothing(small):
    """Budget = the largest job plus one small job (4 pages of 64 at 4 slots): free slots idle until the head of the queue fits."""
    ids, logits, seqs, scores, owner, stats = unpaged(small, 4, 1)
    pt = 64
    needs = [_need(n + N_TOK, pt) for n in LENS]
    budget = (max(needs) + min(needs)) * pt
    pool, seqs_p, scores_p, owner_p = _greedy(small, 4, 1, kv_paged=True, kv_page_tokens=pt, kv_budget_tokens=budget + pt - 1)   # (rounded down)
    assert torch.equal(pool.last_ids, ids) and torch.equal(pool.last_logits, logits) and (seqs_p, owner_p) == (seqs, owner)
    assert pool.stats["kv_pages"] == 1 + max(needs) + min(needs) and pool.stats["kv_pages_peak"] <= max(needs) + min(needs)
    assert pool.stats["kv_page_waits"] > 0 and pool.stats["steps"] > stats["steps"]
    _assert_all_pages_back(pool)
    # the unbudgeted pool of the same call holds more and never waits
    free = _greedy(small, 4, 1, kv_paged=True, kv_page_tokens=pt)[0]
    assert free.stats["kv_page_waits"] == 0 and free.stats["kv_bytes"] > pool.stats["kv_bytes"]


def test_an_oversized_job_is_refused_before_any_forward(small, monkeypatch):
    calls = []
    embed = small.ops.embed
    monkeypatch.setattr(small.ops, "embed", lambda *a, **kw: (calls.append(1), embed(*a, **kw))[1])
    pool = DecodePool(small, TOK, n_slots=2, top_k=1, device="cpu", kv_paged=True, kv_page_tokens=64, kv_budget_tokens=128)
    with pytest.raises(ValueError, match="budget"):
        pool.generate(PROMPTS, n_tokens=N_TOK)                        # prompt 2 needs 3 pages, the budget holds 2
    with pytest.raises(ValueError, match="budget"):
        pool.generate(PROMPTS[:2], n_tokens=[200, 3])                 # the job-control path: prompt 0's own limit
    assert calls == [] and pool.ipd is None
    pool.generate(PROMPTS[:2], n_tokens=N_TOK)                        # what fits runs
    assert calls and pool.stats["kv_pages"] == 3
    _assert_all_pages_back(pool)
    with pytest.raises(ValueError, match="kv_budget_tokens"):
        DecodePool(small, TOK, n_slots=2, device="cpu", kv_paged=True, kv_page_tokens=64, kv_budget_tokens=63)


SEED, TOP_K, TEMP = 11, 4, 10.0                                       # (tests/test_stop_host.py: T = 10 spreads the synthetic model's draws)
MIX = [40] + [3] * (len(PROMPTS) - 1)


def _ctl(m, n_slots, gen, **kw):
    pool = DecodePool(m, TOK, n_slots=n_slots, top_k=TOP_K, top_p=1.0, temperature=TEMP, device="cpu", seed=SEED, allowed_tokens="ACGT", **kw)
    out = pool.generate(PROMPTS, n_sample_per_prompt=N_SPP, **gen)
    return pool, out


CTL_RULES = {
    "limits": dict(n_tokens=MIX),
    "codons": dict(n_tokens=[12] * len(PROMPTS), stop_sequences=["TA", "GG", "CAC"], stop_frame=2),
    "token": dict(n_tokens=MIX, stop_tokens="G"),
    "constraint": dict(n_tokens=[40, 3, 40, 14, 7, 5],
                       constraints=[K.iupac_template("ATGNNRYNTAA"), None, K.encode_protein("MLS*"), K.open_reading_frame(2), None, None]),
    "seeded": dict(n_tokens=N_TOK),                                   # the seeded sampler off the job-control path
}


@pytest.mark.parametrize("budget", [None, "tight"])
@pytest.mark.parametrize("rule", sorted(CTL_RULES))
def test_job_control_and_seeded_paths_equal_the_unpaged_pool(small, rule, budget):
    gen = CTL_RULES[rule]
    want_pool, want = _ctl(small, 3, gen)
    kw = {}
    if budget:
        lim = gen["n_tokens"] if isinstance(gen["n_tokens"], list) else [gen["n_tokens"]] * len(PROMPTS)
        needs = [_need(n + l, 64) for n, l in zip(LENS, lim)]
        kw["kv_budget_tokens"] = (max(needs) + min(needs)) * 64
    pool, got = _ctl(small, 3, gen, kv_paged=True, kv_page_tokens=64, **kw)
    assert got == want
    assert torch.equal(pool.last_ids, want_pool.last_ids) and torch.equal(pool.last_logits, want_pool.last_logits)
    if rule != "seeded":
        assert pool.last_lengths == want_pool.last_lengths and pool.last_finish == want_pool.last_finish
        assert torch.equal(pool.last_logprobs, want_pool.last_logprobs)
        for name in ("stop_ends", "length_ends", "constraint_ends"):
            assert pool.stats.get(name) == want_pool.stats.get(name), name
        if rule in ("codons", "token"):
            assert pool.stats["stop_ends"] > 0                        # jobs did end early: their pages came back before their limit
        if rule == "constraint":
            assert pool.stats["constraint_ends"] > 0
    if budget:
        assert pool.stats["kv_page_waits"] > 0
    _assert_all_pages_back(pool)


def test_sample_many_and_return_logits_false(small):
    kw = dict(n_tokens=4, n_slots=3, n_sample_per_prompt=2, device="cpu", seed=3, return_logits=False, temp=TEMP)
    assert sample_many(PROMPTS[:3], small, TOK, kv_paged=True, kv_page_tokens=64, kv_budget_tokens=256, **kw) == sample_many(PROMPTS[:3], small, TOK, **kw)


# ------------------------------------------------------------------------------------------------ what is refused
def test_what_is_refused(small):
    with pytest.raises(ValueError, match="share_prompt_kv"):
        DecodePool(small, TOK, n_slots=2, device="cpu", kv_paged=True, share_prompt_kv=True)
    with pytest.raises(ValueError, match="kv_dtype"):
        DecodePool(small, TOK, n_slots=2, device="cpu", kv_paged=True, kv_dtype="fp8")
    for pt in (0, 32, 96, 192):
        with pytest.raises(ValueError, match="kv_page_tokens"):
            DecodePool(small, TOK, n_slots=2, device="cpu", kv_paged=True, kv_page_tokens=pt)
    # a backend without the group
    plain = _model(RaggedOracleOps(torch.float64))
    assert not plain.ops.supports("kv_paged") and small.ops.supports("kv_paged")
    with pytest.raises(RuntimeError, match="kv_paged"):
        DecodePool(plain, TOK, n_slots=2, device="cpu", kv_paged=True)
    ids = torch.tensor([list(PROMPTS[1].encode())])
    i = small.attn_layer_idxs[0]

    def paged_cache(m):
        """A prefilled B = 1 cache whose KV entry is swapped for a PagedKV holding the same keys."""
        with torch.inference_mode():
            _, ipd = m(ids, inference_params_dict=m.initialize_inference_params())
        kv = ipd["mha"].key_value_memory_dict[i]
        table = torch.tensor([[1]], dtype=torch.int32)
        rec = PagedKV.zeros(2, 64, m.num_heads, m.head_dim, table, dtype=kv.dtype)
        rec.pages[1, :ids.shape[1]] = kv[0, :ids.shape[1]]
        ipd["mha"].key_value_memory_dict[i] = rec
        ipd["mha"].kv_layout = "paged"
        ipd["mha"].seqlen_offset = ipd["hyena"].seqlen_offset = ids.shape[1]
        return ipd
    with torch.inference_mode():
        ipd = paged_cache(small)
        with pytest.raises(ValueError, match="multi-token forward"):
            small(ids[:, :3], inference_params_dict=ipd)
        with pytest.raises(ValueError, match="scalar-offset step"):
            small(ids[:, :1], inference_params_dict=ipd)
        for field, value in (("shared_prefix", SharedPrefix()), ("prompt_store", PromptStore())):
            ipd = paged_cache(small)
            setattr(ipd["mha"], field, value)
            ipd["mha"].pos_tensor = torch.tensor([ids.shape[1]])
            with pytest.raises(ValueError, match=field):
                small(ids[:, :1], inference_params_dict=ipd)
        # the per-row step itself runs, and equals the contiguous step
        ipd = paged_cache(small)
        ipd["mha"].pos_tensor = torch.tensor([ids.shape[1]])
        got = small(ids[:, :1], inference_params_dict=ipd)[0]
        _, ref = small(ids, inference_params_dict=small.initialize_inference_params())
        ref["mha"].seqlen_offset = ref["hyena"].seqlen_offset = ids.shape[1]
        ref["mha"].pos_tensor = torch.tensor([ids.shape[1]])
        ref["mha"].key_value_memory_dict[i] = torch.cat([ref["mha"].key_value_memory_dict[i], torch.zeros_like(ref["mha"].key_value_memory_dict[i])], 1)
        assert torch.equal(got, small(ids[:, :1], inference_params_dict=ref)[0])
        # a backend without the group, at the model's door
        ipd = paged_cache(plain)
        ipd["mha"].pos_tensor = torch.tensor([ids.shape[1]])
        with pytest.raises(RuntimeError, match="kv_paged"):
            plain(ids[:, :1], inference_params_dict=ipd)
        # the layout named without the record, and the record without the layout's name
        ipd = paged_cache(small)
        ipd["mha"].kv_layout = "contiguous"
        ipd["mha"].pos_tensor = torch.tensor([ids.shape[1]])
        with pytest.raises(ValueError, match="kv_layout"):
            small(ids[:, :1], inference_params_dict=ipd)
        # _kv_buffer never allocates or grows a paged cache
        ipd = paged_cache(small)
        with pytest.raises(ValueError, match="never grown"):
            small._kv_buffer(ipd["mha"], i, 1, 4096, ids)
    assert not small._graph_eligible(paged_cache(small))


# ------------------------------------------------------------------------------------------------ resources
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_paged_kernels_need_no_scratch_and_stay_inside_the_siblings_registers():
    meta = _metadata("kv_paged.hip")
    kernels = {k: r for k, r in meta.items() if any(n in k for n in ("rope_append_decode_paged_kernel", "attn_decode_paged_kernel"))}
    assert len(kernels) == 2 == len(meta), sorted(meta)
    for name, r in kernels.items():
        assert r["scratch"] == 0 and r["spill"] == 0 and r["sgpr_spill"] == 0 and r["lds"] == 0, (name, r)
    attn = next(r for k, r in kernels.items() if "attn_decode_paged_kernel" in k)
    sibling = next(r for k, r in _metadata("attn.hip").items() if "attn_decode_stream_kernel" in k)
    print(f"[paged kv] attn_decode_paged_kernel {attn}; attn_decode_stream_kernel {sibling}")
    assert attn["vgpr"] <= 256, attn                                  # two waves per SIMD, as the sibling
    assert attn["vgpr"] <= sibling["vgpr"] + 8, (attn, sibling)
