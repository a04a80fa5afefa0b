"""CPU: the host side of the decode pool's opt-in batch-invariant step on the oracle backend -- what is refused and
when, where the flag travels, that the pool with the option still generates what per-prompt greedy `generate` does, and that a pool
WITHOUT the option asks its backend for exactly what it asked before.  The kernels' own statements (row invariance, exactness) need the
GPU: tests/test_gpu_rowinv.py, tests/test_gpu_rowinv_rows.py, tests/test_gpu_step_rows.py, tests/test_gpu_batch_invariant.py.  Their CPU
companion is at the end of this module: the routing of the row-invariant launches restated in plain Python (tests/rowinv_ref.py), held
to the source, to the figures DESIGN.md section 25 quotes and to the shapes those GPU modules run."""
import os
import re

import pytest
import torch

from evo_amd import _build
from evo_amd import ops as evo_ops
from evo_amd.backend import Backend
from evo_amd.generation import generate
from evo_amd.pool import DecodePool, sample_many
from test_gpu_pool import PROMPTS
from test_kernel_resources import HIPCC, _metadata
from test_paged_kv_host import PagedCtlOps, _model
from test_ragged_prefill_host import TOK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("evo_linear_rowinv_bf16", "evo_mlp_gate_rowinv_bf16")
HOST_FUNCTIONS = {"supports", "adopt"} | {n for n, v in vars(Backend).items() if isinstance(v, staticmethod)}


class RowInvOps:
    """The group "row_invariant" on an oracle backend: in fp64 every summation order gives the same sums, so the three methods ARE the
    plain ones (the property they add exists on the GPU only)."""

    def linear_rowinv(self, x, w, b=None):
        return self.linear(x, w, b)

    def linear_residual_rowinv_(self, res, x, w, bias=None):
        return self.linear_residual_(res, x, w, bias=bias)

    def mlp_gate_rowinv(self, x, w12, w12g=None):
        return self.gelu_gate(self.linear(x, w12, None))


class Recording:
    """Every backend method the host calls, by name and in order, in `self.log` (calls a method makes on itself included)."""

    def __getattribute__(self, name):
        attr = object.__getattribute__(self, name)
        if name.startswith("_") or name in HOST_FUNCTIONS or not callable(attr):
            return attr
        log = object.__getattribute__(self, "log")

        def logged(*a, **kw):
            log.append(name)
            return attr(*a, **kw)
        return logged


class OldOps(Recording, PagedCtlOps):
    """The oracle backend as it was before the group existed."""

    def __init__(self):
        object.__setattr__(self, "log", [])
        super().__init__(torch.float64)


class NewOps(Recording, RowInvOps, PagedCtlOps):
    def __init__(self):
        object.__setattr__(self, "log", [])
        super().__init__(torch.float64)


@pytest.fixture(scope="module")
def small():
    return _model(NewOps())


N_TOK = 6


def test_entries_are_wired():
    header = open(os.path.join(ROOT, "include", "evo_mi355x.h")).read()
    for name in ENTRIES:
        assert name in _build.EXPORTS and name in evo_ops._SIGNATURES and re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert int(re.search(r"#define EVO_ABI_VERSION (\d+)", header).group(1)) == evo_ops.ABI_VERSION >= 20
    assert Backend.OPTIONAL["row_invariant"] == ("linear_rowinv", "linear_residual_rowinv_", "mlp_gate_rowinv")
    assert all(hasattr(evo_ops.HipOps, n) for n in Backend.OPTIONAL["row_invariant"])
    assert "csrc/gemv_inv.hip" in "".join(str(p) for p in _build.sources()).replace(os.sep, "/")


def test_what_is_refused_before_the_backend_sees_a_call(small):
    small.ops.log.clear()
    kw = dict(device="cpu", batch_invariant=True)
    for match, bad in (("n_slots", dict(n_slots=65)), ("prefill_batch", dict(n_slots=2, prefill_batch=2)),
                       ("share_prompt_kv", dict(n_slots=2, share_prompt_kv=True)), ("kv_dtype", dict(n_slots=2, kv_dtype="fp8")),
                       ("weight_dtype", dict(n_slots=2, weight_dtype="fp8"))):
        with pytest.raises(ValueError, match=match):
            DecodePool(small, TOK, **bad, **kw)
        assert small.ops.log == [], (match, small.ops.log)
    with pytest.raises(ValueError, match="batch_invariant"):
        sample_many(PROMPTS[:2], small, TOK, n_tokens=2, n_slots=2, device="cpu", prefill_batch=2, batch_invariant=True)
    pool = DecodePool(small, TOK, n_slots=4, allowed_tokens="ACGT", **kw)
    with pytest.raises(ValueError, match="batch_invariant"):
        pool.beam_search(PROMPTS[:1], n_tokens=2, beam_width=2)
    assert small.ops.log == [] and pool.ipd is None and pool.stats["batch_invariant"] is True
    DecodePool(small, TOK, n_slots=64, **kw)                                            # 64 slots are served
    assert DecodePool(small, TOK, n_slots=2, device="cpu").stats["batch_invariant"] is False
    # a backend without the group
    old = _model(OldOps())
    assert not old.ops.supports("row_invariant") and small.ops.supports("row_invariant")
    with pytest.raises(RuntimeError, match="row_invariant"):
        DecodePool(old, TOK, n_slots=2, **kw)
    assert old.ops.log == []
    # ... and the model's own door: a cache record that asks for the step on such a backend, or with more rows than the launches serve
    ids = torch.tensor([list(PROMPTS[1].encode())])
    _, ipd = old(ids, inference_params_dict=old.initialize_inference_params())
    ipd["mha"].batch_invariant = True
    ipd["mha"].seqlen_offset = ipd["hyena"].seqlen_offset = ids.shape[1]
    with pytest.raises(RuntimeError, match="row_invariant"):
        old(ids[:, -1:], inference_params_dict=ipd)
    _, ipd = small(ids, inference_params_dict=small.initialize_inference_params())
    ipd["mha"].batch_invariant = True
    ipd["mha"].seqlen_offset = ipd["hyena"].seqlen_offset = ids.shape[1]
    with pytest.raises(ValueError, match="per-row single-token step"):                  # Generator's scalar-offset step is out of scope
        small(ids[:, -1:], inference_params_dict=ipd)


def test_the_flag_reaches_every_single_token_block_and_no_prefill(small, monkeypatch):
    pool = DecodePool(small, TOK, n_slots=3, top_k=1, temperature=0.0, device="cpu", batch_invariant=True)
    seen = []

    def spy(name, cache_arg):
        inner = getattr(small, name)

        def wrapped(*a, **kw):
            T = a[cache_arg - 1]
            cache = a[cache_arg]
            own = pool.ipd is not None and cache in (pool.ipd["mha"], pool.ipd["hyena"])
            seen.append((name, T, own, bool(kw.get("inv", False))))
            return inner(*a, **kw)
        monkeypatch.setattr(small, name, wrapped)
    spy("_hyena_block", 5)                                                             # (i, blk, x2d, B, T, cache, ...)
    spy("_attn_block", 5)
    mlp_inv = []
    mlp = small._mlp_residual_
    monkeypatch.setattr(small, "_mlp_residual_", lambda *a, **kw: (mlp_inv.append((a[1].shape[0], bool(kw.get("inv", False)))), mlp(*a, **kw))[1])
    small.ops.log.clear()
    pool.generate(PROMPTS, n_tokens=N_TOK)                                              # (PROMPTS[3] is one token: a T = 1 PREFILL)
    steps = [s for s in seen if s[2]]
    prefills = [s for s in seen if not s[2]]
    assert len(steps) == small.num_layers * pool.stats["steps"] > 0 and len(prefills) == small.num_layers * len(PROMPTS)
    assert all(T == 1 and inv for _, T, _, inv in steps), "a block of the pooled step ran without the flag"
    assert not any(inv for _, _, _, inv in prefills), "a prefill saw the flag"
    assert any(T == 1 for _, T, _, _ in prefills)
    assert sum(inv for _, inv in mlp_inv) == len(steps) and all(rows == 3 for rows, inv in mlp_inv if inv)
    # the step's launch sequence holds no fused and no row-count-routed dense call
    log = small.ops.log
    n_steps, L = pool.stats["steps"], small.num_layers
    assert log.count("mlp_gate_rowinv") == L * n_steps and log.count("linear_residual_rowinv_") == 2 * L * n_steps
    assert log.count("linear_rowinv") == (L + 1) * n_steps                              # every block's projection + the unembedding
    assert log.count("hyena_step") == len(small.hyena_layer_idxs) * n_steps and "hyena_decode_fused" not in log


@pytest.mark.parametrize("n_slots", [1, 3, 9])
def test_pool_with_the_option_equals_per_prompt_greedy_generate(small, n_slots):
    want, _ = generate(PROMPTS, small, TOK, n_tokens=N_TOK, temperature=0.0, top_k=1, batched=False, cached_generation=True, verbose=0,
                       device="cpu")
    pool = DecodePool(small, TOK, n_slots=n_slots, top_k=1, top_p=1.0, temperature=0.0, device="cpu", batch_invariant=True)
    seqs, scores, owner = pool.generate(PROMPTS, n_tokens=N_TOK)
    assert owner == list(range(len(PROMPTS))) and seqs == want
    paged = DecodePool(small, TOK, n_slots=n_slots, top_k=1, top_p=1.0, temperature=0.0, device="cpu", batch_invariant=True, kv_paged=True,
                       kv_page_tokens=64)
    assert paged.generate(PROMPTS, n_tokens=N_TOK)[0] == want


def test_a_default_pool_asks_its_backend_for_what_it_asked_before(small):
    """The same run on the backend as it was (no group) and on the one with the group: one sequence of backend calls, and none of the new ones."""
    old = _model(OldOps())
    logs = {}
    for name, m in (("old", old), ("new", small)):
        m.ops.log.clear()
        pool = DecodePool(m, TOK, n_slots=3, top_k=4, temperature=10.0, device="cpu", seed=11, allowed_tokens="ACGT")
        out = pool.generate(PROMPTS, n_tokens=[9, 3, 4, 5, 3, 3], n_sample_per_prompt=2, stop_tokens="G")
        logs[name] = (list(m.ops.log), out, pool.last_ids.clone(), pool.last_logits.clone())
    assert logs["old"][0] == logs["new"][0] and len(logs["new"][0]) > 100
    assert not any(n in logs["new"][0] for n in Backend.OPTIONAL["row_invariant"]) and "hyena_decode_fused" in logs["new"][0]
    assert logs["old"][1] == logs["new"][1] and torch.equal(logs["old"][2], logs["new"][2]) and torch.equal(logs["old"][3], logs["new"][3])


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_rowinv_kernels_need_no_scratch():
    kernels = _metadata("gemv_inv.hip")
    nw = {k: v for k, v in kernels.items() if "skinny_nw_kernel" in k}
    # wide: 4 m tiles x 2 / 3 / 4 waves; split over K: 4 m tiles x 2 / 4 waves; gate: 4 m tiles
    assert len(nw) == 12 + 8 + 4 and any("skinny_reduce_kernel" in k for k in kernels), sorted(kernels)
    for name, r in kernels.items():
        assert r["spill"] == 0 and r["scratch"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["lds"] <= 160 * 1024 and r["vgpr"] <= 256, (name, r)                   # (a CU holds 160 KiB of LDS)


# ================================================================================================ the routing, restated (tests/rowinv_ref.py)
import rowinv_ref as RI  # noqa: E402


def _rowinv_source():
    src = open(os.path.join(ROOT, "evo_amd", "csrc", "gemv_inv.hip")).read() + open(os.path.join(ROOT, "evo_amd", "csrc", "skinny_nw.h")).read()
    return re.sub(r"\s+", " ", src)


def test_the_restatement_reads_like_the_source():
    """The constants the restatement is built from, where the source states them (a change of the rule has to touch both)."""
    src = _rowinv_source()
    for needle in ("if (N >= 8192) {", "const int64_t groups = N / (N < 2048 ? 32 : 64);", "int64_t slices = (256 + groups - 1) / groups;",
                   "if (slices > K / 256) slices = K / 256;", "return slices > 8 ? 8 : slices;",
                   "if (N >= 256 * 64) launch(mt, gv_int<4>{}); else if (N >= 256 * 48) launch(mt, gv_int<3>{}); else launch(mt, gv_int<2>{});",
                   "if (N < 2048) launch(mt, gv_int<2>{}); else launch(mt, gv_int<4>{});", "constexpr int KC = MT <= 2 ? 8 : 4;",
                   "constexpr int CPU = 8 / KC;", "const int n_cut = SLICE256 ? n_chunk_all / CPU : n_chunk_all, cut = SLICE256 ? CPU : 1;",
                   "(int)((int64_t)n_cut * blockIdx.y / gridDim.y) * cut",
                   "skinny_nw_kernel<decltype(mt)::value, WV, true, false, true>",
                   "if (M <= 16) f(gv_int<1>{}); else if (M <= 32) f(gv_int<2>{}); else if (M <= 48) f(gv_int<3>{}); else f(gv_int<4>{});"):
        assert needle in src, needle
    assert [RI.mt_of(M) for M in (1, 16, 17, 32, 33, 48, 49, 64)] == [1, 1, 2, 2, 3, 3, 4, 4] and [RI.kc_of(t) for t in (1, 2, 3, 4)] == [8, 8, 4, 4]


def test_slices_do_not_move_with_the_chunk_length_under_the_256_k_cut():
    """Every K that is a multiple of 256 up to 11,008 and every slice count 1 .. min(8, K / 256): cut in 256-k units the boundaries are the
    same at both chunk lengths; cut in chunks (the default SPLITK) they differ for 202 pairs, (11008, 4) among them -- 2,560 against
    2,688, the figure DESIGN.md section 25 quotes."""
    cuts = RI.all_cuts()
    assert len(cuts) == 316 and cuts[0] == (256, 1) and cuts[-1] == (11008, 8)
    for K, s in cuts:
        for unit256 in (True, False):
            for kc in (8, 4):
                b = RI.boundaries(K, s, kc, unit256)
                assert b[0] == 0 and b[-1] == K and b == sorted(b) and all(v % (32 * kc) == 0 for v in b), (K, s, kc, unit256, b)
        assert all(v % 256 == 0 for v in RI.boundaries(K, s, 4, True))
    assert [c for c in cuts if RI.boundaries(*c, 8, True) != RI.boundaries(*c, 4, True)] == []
    differ = [c for c in cuts if RI.boundaries(*c, 8, False) != RI.boundaries(*c, 4, False)]
    assert len(differ) == 202 and (11008, 4) in differ
    assert RI.boundaries(11008, 4, 8, False)[1] == 2560 and RI.boundaries(11008, 4, 4, False)[1] == 2688
    assert RI.boundaries(11008, 4, 8, True) == RI.boundaries(11008, 4, 4, True) == [0, 2560, 5376, 8192, 11008]
    # what a build without the 256-k cut would show to tests/test_gpu_rowinv_rows.py (M >= 33 against the one-row call): the shapes
    # whose boundaries move, and the two 7B shapes whose boundaries do not
    moves = {(N, K): RI.boundaries(K, RI.rowinv_slices(N, K), 8, False) != RI.boundaries(K, RI.rowinv_slices(N, K), 4, False)
             for N, K in RI.LINEAR_7B + RI.LINEAR_SMALL if N < RI.WIDE_N}
    assert moves == {(4096, 4096): False, (4096, 11008): True, (512, 4096): False, (512, 2304): True, (4096, 2816): True}
    src = open(os.path.join(ROOT, "DESIGN.md")).read()
    assert "k = 2,560 up to 32 rows and at 2,688 from 33" in src


def test_routes_of_the_test_shapes():
    assert (RI.route(12288, 4096), RI.rowinv_slices(12288, 4096)) == ("wide3", 0)
    assert (RI.route(4096, 4096), RI.slice_units(4096, 4096)) == ("split4", [4, 4, 4, 4])
    assert (RI.route(4096, 11008), RI.slice_units(4096, 11008)) == ("split4", [10, 11, 11, 11])
    assert (RI.route(512, 4096), RI.slice_units(512, 4096)) == ("split2", [2] * 8)
    assert (RI.route(512, 2304), RI.slice_units(512, 2304)) == ("split2", [1] * 7 + [2])
    assert (RI.route(4096, 2816), RI.slice_units(4096, 2816)) == ("split4", [2, 3, 3, 3])
    assert [RI.route(N, 256) for N in (8192, 12288, 16384)] == ["wide2", "wide3", "wide4"]
    # the existing module's shapes (tests/test_gpu_rowinv.py SHAPES), for the record
    assert [(RI.route(N, K), RI.rowinv_slices(N, K)) for N, K in ((8192, 256), (16384, 256), (2048, 512), (4096, 1792), (512, 512))] == \
        [("wide2", 0), ("wide4", 0), ("split4", 2), ("split4", 4), ("split2", 2)]
    assert RI.slice_units(4096, 1792) == [1, 2, 2, 2]
    # the workspace the binding hands over (8 M N floats) always suffices
    assert all(0 <= RI.rowinv_slices(N, K) <= 8 for N in range(64, 16448, 64) for K in (256, 2304, 4096, 11008))


def test_every_route_meets_every_m_tile_count_in_the_gpu_modules():
    """Every route (2 / 3 / 4 waves wide; 2 / 4 waves split over K; gate) x every MT (1 .. 4) is reached by some (shape, M) the every-M
    tests of tests/test_gpu_rowinv_rows.py run -- the lists are the restatement's own, which that module imports."""
    cases = [(N, K, M) for N, K in RI.LINEAR_7B + RI.LINEAR_SMALL for M in RI.EVERY_M]
    got = RI.reached(cases, RI.EVERY_M)
    assert got == {(r, t) for r in RI.ROUTES for t in (1, 2, 3, 4)}, sorted({(r, t) for r in RI.ROUTES for t in (1, 2, 3, 4)} - got)
    assert {RI.route(N, K) for N, K in RI.LINEAR_7B} == {"wide3", "split4", "split2"}
    mod = open(os.path.join(ROOT, "tests", "test_gpu_rowinv_rows.py")).read()
    assert "SHAPES = RI.LINEAR_7B + RI.LINEAR_SMALL" in mod and "GATES = [RI.GATE_7B]" in mod and "for M in RI.EVERY_M" in mod
