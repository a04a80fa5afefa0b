"""CPU: the decode pool with ONE stored K/V per prompt (DecodePool share_prompt_kv) -- the layers that need no GPU.

  * the pool on the fp64 oracle backend (tests/oracle_ops.OracleOps plus `attention_decode_prefix` by concatenation, the pattern of
    tests/test_variants_host.PrefixOracleOps): greedy runs with and without sharing agree in every token and every logit, by
    torch.equal -- the concatenation hands the oracle the very keys the replicated cache holds, in the same order;
  * the host bookkeeping: one K/V install per prompt, own caches of n_tokens rows, the store-row formula, reference counts back at 0;
  * the new C entries: exported, ABI 15, and every contract violation of include/evo_mi355x.h refused with -1 before any launch
    (null or never-dereferenced pointers: no GPU needed);
  * resources: attn_decode_group_kernel without scratch inside 512 registers; the two kernels it shares a launch sequence with still
    without scratch."""
import ctypes
import os
import re

import pytest
import torch

from evo_amd import _build
from evo_amd import ops as evo_ops
from evo_amd.pool import DecodePool
from evo_amd.tokenizer import CharLevelTokenizer
from oracle_ops import OracleOps
from test_gpu_pool import PROMPTS
from test_kernel_resources import HIPCC, _metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOK = CharLevelTokenizer(512)
SMALL = dict(vocab_size=512, hidden_size=256, num_layers=4, attn_layer_idxs=[2], num_attention_heads=2)   # tests/test_gpu_embed.SMALL
N_TOK = 6


class FanoutOracleOps(OracleOps):
    """OracleOps + the decode attention behind a prompt store, by concatenation."""
    attn_group_rows = evo_ops.ATTN_GROUP_ROWS

    def __init__(self, act=torch.float64):
        super().__init__(act)
        self.prefix_calls = 0

    def attention_decode_prefix(self, q, k, v, own_pos, k_store, v_store, pre_row, pre_len, n_splits=None, n_pre_splits=None,
                                prescaled=False):
        assert not prescaled
        self.prefix_calls += 1
        rows = []
        for b in range(q.shape[0]):
            r, n = int(pre_row[b]), int(own_pos[b]) + 1
            P = int(pre_len[r]) if r >= 0 else 0
            kc = torch.cat([k_store[r, :P], k[b, :n]], 0)[None]
            vc = torch.cat([v_store[r, :P], v[b, :n]], 0)[None]
            rows.append(self.attention_decode(q[b:b + 1], kc, vc))
        return torch.cat(rows, 0)


@pytest.fixture(scope="module")
def small():
    from oracle.stripedhyena_ref import RefConfig, make_synthetic_state_dict
    from evo_amd.sh.model import StripedHyena
    sd = make_synthetic_state_dict(RefConfig.from_dict(SMALL), seed=3)
    m = StripedHyena(dict(SMALL), ops=FanoutOracleOps(torch.float64))
    m.load_state_dict({k: (v.double() if v.dtype == torch.bfloat16 else v) for k, v in sd.items()})
    return m


def _pool(m, n_slots, share):
    return DecodePool(m, TOK, n_slots=n_slots, top_k=1, top_p=1.0, temperature=0.0, device="cpu", share_prompt_kv=share)


@pytest.fixture(scope="module")
def replicated(small):
    """The yardstick, computed once per slot count: the pool as it is without the option."""
    out = {}
    for n_slots in (4, 8):
        pool = _pool(small, n_slots, False)
        seqs, scores, owner = pool.generate(PROMPTS, n_tokens=N_TOK, n_sample_per_prompt=3)
        out[n_slots] = (pool.last_ids.clone(), pool.last_logits.clone(), seqs, scores, owner)
    return out


@pytest.mark.parametrize("n_slots", [4, 8])
def test_shared_pool_equals_the_replicated_pool(small, replicated, n_slots):
    want_ids, want_logits, want_seqs, want_scores, want_owner = replicated[n_slots]
    small.ops.prefix_calls = 0
    pool = _pool(small, n_slots, True)
    seqs, scores, owner = pool.generate(PROMPTS, n_tokens=N_TOK, n_sample_per_prompt=3)
    assert small.ops.prefix_calls == pool.stats["steps"] > 0            # one attention layer: the new path ran, every step
    assert owner == want_owner and seqs == want_seqs and scores == want_scores
    assert torch.equal(pool.last_ids, want_ids)
    assert torch.equal(pool.last_logits, want_logits)
    # bookkeeping
    assert pool.stats["prefills"] == len(PROMPTS)
    assert pool.stats["prompt_kv_installs"] == len(PROMPTS)              # (the replicated path installs once per JOB: 18 copies)
    R = min(n_slots, -(-n_slots // 3) + 1)
    assert pool.stats["store_rows"] == R == len(pool.store_refs) and R == {4: 3, 8: 4}[n_slots]
    p_max = max(len(p) for p in PROMPTS)
    for i in small.attn_layer_idxs:
        assert tuple(pool.ipd["mha"].key_value_memory_dict[i].shape[:2]) == (n_slots, N_TOK)     # only what a slot generates
        assert tuple(pool.store.kv[i].shape[:2]) == (R, p_max)
    assert pool.store_refs == [0] * R and pool.store.row.tolist() == [-1] * n_slots
    # every step streams at least one store row per tile that holds a live slot and at most one per live slot
    assert pool.stats["steps"] <= pool.stats["prefix_streams"] <= pool.stats["tokens"]


def test_one_sample_per_prompt_puts_every_slot_on_its_own_store_row(small):
    ref = _pool(small, 4, False)
    ref.generate(PROMPTS, n_tokens=N_TOK)
    pool = _pool(small, 4, True)
    rows_seen = []
    install = pool._install_shared

    def spy(slot, pi, tmp, P):
        install(slot, pi, tmp, P)
        live = [r for r in pool._slot_row if r >= 0]
        assert len(live) == len(set(live))                               # no two live slots share a row
        rows_seen.append(pool._slot_row[slot])
    pool._install_shared = spy
    pool.generate(PROMPTS, n_tokens=N_TOK)
    assert torch.equal(pool.last_ids, ref.last_ids) and torch.equal(pool.last_logits, ref.last_logits)
    assert pool.stats["store_rows"] == 4 and pool.stats["prompt_kv_installs"] == len(PROMPTS) == len(rows_seen)
    assert pool.store_refs == [0] * 4
    assert pool.stats["prefix_streams"] == pool.stats["tokens"]          # a stream per live slot and step


def test_single_token_jobs_and_pool_reuse(small):
    pool = _pool(small, 3, True)
    one, _, _ = pool.generate(PROMPTS[:3], n_tokens=1, n_sample_per_prompt=2)       # every stream ends at its prefill
    assert len(one) == 6 and pool.store_refs == [0] * len(pool.store_refs)
    ref = _pool(small, 3, False)
    ref.generate(PROMPTS[:4], n_tokens=N_TOK, n_sample_per_prompt=2)
    pool.generate(PROMPTS[:4], n_tokens=N_TOK, n_sample_per_prompt=2)               # a longer job on the same pool: caches re-made
    assert torch.equal(pool.last_ids, ref.last_ids) and torch.equal(pool.last_logits, ref.last_logits)
    assert pool.store_refs == [0] * len(pool.store_refs)


def test_a_backend_without_the_kernel_is_refused():
    class Plain:
        ops = OracleOps()
    with pytest.raises(RuntimeError, match="attention_decode_prefix"):
        DecodePool(Plain(), TOK, n_slots=2, device="cpu", share_prompt_kv=True)
    DecodePool(Plain(), TOK, n_slots=2, device="cpu")                    # the default asks for nothing new


# ------------------------------------------------------------------------------------------------ C ABI
def test_new_entries_are_exported_and_refuse_before_any_launch():
    header = open(os.path.join(ROOT, "include", "evo_mi355x.h")).read()
    for name in ("evo_attn_decode_prefix_bf16", "evo_rope_append_decode_at_bf16"):
        assert name in _build.EXPORTS and name in evo_ops._SIGNATURES and re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert int(re.search(r"#define EVO_ABI_VERSION (\d+)", header).group(1)) == evo_ops.ABI_VERSION >= 15
    assert int(re.search(r"#define EVO_ATTN_GROUP_ROWS (\d+)", header).group(1)) == evo_ops.ATTN_GROUP_ROWS == evo_ops.HipOps.attn_group_rows
    lib = evo_ops.load_library()
    one = ctypes.c_void_p(16)                                            # non-null, aligned, never dereferenced
    H, cap, P_cap = 2, 64, 128
    row = 2 * H * 128                                                    # token stride of a [.., cap, 2, H, 128] cache

    def call(**kw):
        a = dict(q=one, k=one, v=one, o=one, B=3, H=H, Tk=cap, q_sb=3 * H * 128, q_sh=128, k_sb=cap * row, k_st=row, k_sh=128,
                 v_sb=cap * row, v_st=row, v_sh=128, own_pos=one, k_pre=one, v_pre=one, R=2, P_cap=P_cap, kp_sb=P_cap * row, kp_st=row,
                 kp_sh=128, vp_sb=P_cap * row, vp_st=row, vp_sh=128, pre_row=one, pre_len=one, part_o=one, part_ml=one, n_pre=4, n_own=4)
        a.update(kw)
        return lib.evo_attn_decode_prefix_bf16(
            a["q"], a["k"], a["v"], a["o"], a["B"], a["H"], a["Tk"], a["q_sb"], a["q_sh"], a["k_sb"], a["k_st"], a["k_sh"], a["v_sb"],
            a["v_st"], a["v_sh"], a["own_pos"], a["k_pre"], a["v_pre"], a["R"], a["P_cap"], a["kp_sb"], a["kp_st"], a["kp_sh"], a["vp_sb"],
            a["vp_st"], a["vp_sh"], a["pre_row"], a["pre_len"], a["part_o"], a["part_ml"], a["n_pre"], a["n_own"], 1.0, None)

    for name in ("q", "k", "v", "o", "own_pos", "k_pre", "v_pre", "pre_row", "pre_len", "part_o", "part_ml"):
        assert call(**{name: None}) == -1, name                          # null pointers
    assert call(R=0) == -1 and call(n_pre=0) == -1 and call(n_pre=-4) == -1
    assert call(n_pre=1000, n_own=25) == -1 and call(n_pre=1, n_own=1024) == -1          # more than 1,024 splits in all
    for name in ("q_sb", "q_sh", "k_sb", "k_st", "k_sh", "v_sb", "v_st", "v_sh", "kp_sb", "kp_st", "kp_sh", "vp_sb", "vp_st", "vp_sh"):
        assert call(**{name: 516}) == -1, name                           # a stride that is no multiple of 8
    # 32-bit key offsets: capacity x token stride x 2 bytes at or above 2^32 - 1 -- store and own cache alike; no other form exists
    big = 1 << 20                                                        # token stride in elements (2 MiB)
    assert call(P_cap=2048, kp_st=big) == -1 and call(P_cap=2048, vp_st=big) == -1
    assert call(Tk=2048, k_st=big) == -1 and call(Tk=2048, v_st=big) == -1
    assert call(P_cap=262144, kp_st=8192, vp_st=8192) == -1              # 262,144 keys at H = 32: exactly 2^32 bytes
    # the rotary entry: the existing refusals, and a null widx
    f1 = ctypes.c_float(1.0)
    at = lib.evo_rope_append_decode_at_bf16
    assert at(one, one, one, one, f1, 1, 32, 128, 8, 8, 8, 8, f1, None, None) == -1
    assert at(None, one, one, one, f1, 1, 32, 128, 8, 8, 8, 8, f1, one, None) == -1
    assert at(one, one, one, one, f1, 1, 32, 128, 8, 12, 8, 8, f1, one, None) == -1
    assert at(one, one, one, one, f1, 1, 32, 120, 8, 8, 8, 8, f1, one, None) == -1


# ------------------------------------------------------------------------------------------------ resources
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_grouped_decode_kernel_needs_no_scratch():
    meta = _metadata("attn.hip")
    group = {k: v for k, v in meta.items() if "attn_decode_group_kernel" in k}
    assert len(group) == 1, sorted(group)                                # one shipped form
    for name, r in group.items():
        print(name, r)
        assert r["scratch"] == 0 and r["vgpr"] <= 512 and r["lds"] == 0, (name, r)
    for pattern in ("attn_decode_stream_kernel", "attn_decode_combine_kernel"):
        ks = {k: v for k, v in meta.items() if pattern in k}
        assert len(ks) == 1, sorted(ks)
        for name, r in ks.items():
            assert r["scratch"] == 0, (name, r)
