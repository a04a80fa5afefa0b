"""CPU: variant-effect scoring from cached prefixes -- the layers that need no GPU.

  * plan_variants on a hand-written table (exact first differences, checkpoints and groups);
  * score_variants end to end on the fp64 oracle backend (tests/oracle_ops.OracleOps plus `attention_prefix` by concatenation)
    against full forwards of every variant on the same ops.  Bound: tests/test_oracle.test_cached_decode_matches_full_forward
    holds a cached continuation to the stateless forward within 1e-9 per position on this oracle; a delta sums the log-probs of
    up to T positions, so the bound here is 1e-9 x (number of summed positions).  The full-forward side takes its log-softmax in
    fp64 (score_sequences' host path rounds its log-softmax to fp32, 6e-8 x |lp| per position, which would hide a 1e-9 bound);
    score_sequences itself is then held to the fp32 bound of tests/test_profile_host.py (4e-4 per position);
  * the new C entries: exported, refuse illegal shapes before any launch, and the new kernel instantiations stay in their budget
    (no scratch, no VGPR spill, LDS = W_LDS)."""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import numpy as np
import pytest
import torch

from evo_amd import _build
from evo_amd import ops as evo_ops
from evo_amd.scoring import VARIANT_MIN_SUFFIX, first_difference, plan_variants, score_sequences, score_variants, single_substitutions
from evo_amd.tokenizer import CharLevelTokenizer
from oracle_ops import OracleOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
TOK = CharLevelTokenizer(512)
SMALL = dict(vocab_size=512, hidden_size=256, num_layers=4, attn_layer_idxs=[2], num_attention_heads=2)   # tests/test_gpu_embed.SMALL
W_LDS = 4 * 64 * 272 + 3 * 64 * 256


# ------------------------------------------------------------------------------------------------ planner
def _ids(n, seed=0):
    return list(np.random.default_rng(seed).integers(1, 5, size=n))


def _sub(ids, i):
    out = list(ids)
    out[i] = 9
    return out


def test_planner_on_a_hand_written_table():
    E = 64
    ref = [0] + _ids(400)                                   # T = 401 tokens (BOS + 400)
    table = [                                               # (variant ids, first_diff, checkpoint)
        (_sub(ref, 1), 1, 0),                               # d = 1
        (_sub(ref, 64), 64, 0),                             # d - 1 = 63: one short of the checkpoint
        (_sub(ref, 65), 65, 64),                            # d - 1 exactly on a checkpoint
        (_sub(ref, 66), 66, 64),                            # ... and one past it
        (_sub(ref, 300), 300, 256),                         # 401 - 256 = 145 >= 129
        (_sub(ref[:385], 300), 300, 256),                   # suffix of exactly 129 tokens at c = 256
        (_sub(ref[:384], 300), 300, 192),                   # suffix of 128 at c = 256: one checkpoint back (384 - 192 = 192)
        (_sub(ref, 400), 400, 256),                         # last token: 401 - 320 = 81 < 129, 401 - 256 = 145
        (ref[:200] + [7, 7, 7] + ref[200:], 200, 192),      # insertion
        (ref[:200] + ref[202:], None, 192),                 # deletion (first difference found below)
        (ref[:350], 350, 192),                              # truncation: a prefix -> d = its length; 350 - 320 < 129, 350 - 256 < 129
        (list(ref), -1, -1),                                # a copy of the reference
    ]
    dels = first_difference(ref, table[9][0])
    assert 200 <= dels < 210
    table[9] = (table[9][0], dels, 192)
    plan = plan_variants(ref, [t[0] for t in table], checkpoint_every=E, max_batch_tokens=1 << 30, max_rows_per_pass=64)
    assert plan.first_diff.tolist() == [t[1] for t in table]
    assert plan.checkpoint.tolist() == [t[2] for t in table]
    assert plan.checkpoints == (64, 192, 256)
    assert [(g.checkpoint, g.index) for g in plan.groups] == [(0, (0, 1)), (64, (2, 3)), (192, (6, 8, 9, 10)), (256, (4, 5, 7))]
    assert [(g.rows, g.width) for g in plan.groups] == [(3, 401), (3, 337), (5, 212), (4, 145)]
    assert plan.tokens == 401 + 3 * 401 + 3 * 337 + 5 * 212 + 4 * 145
    assert plan.naive_tokens == 13 * 404
    for g in plan.groups:
        assert g.checkpoint == 0 or g.width >= VARIANT_MIN_SUFFIX
    # passes are cut by rows and by rows x width
    p2 = plan_variants(ref, [t[0] for t in table], checkpoint_every=E, max_batch_tokens=1 << 30, max_rows_per_pass=3)
    assert [(g.checkpoint, g.index) for g in p2.groups] == [(0, (0, 1)), (64, (2, 3)), (192, (6, 8)), (192, (9, 10)), (256, (4, 5)), (256, (7,))]
    p3 = plan_variants(ref, [t[0] for t in table], checkpoint_every=E, max_batch_tokens=3 * 212, max_rows_per_pass=64)
    assert all(g.rows * g.width <= 3 * 212 or g.rows == 2 for g in p3.groups)
    assert sorted(n for g in p3.groups for n in g.index) == list(range(11))
    for bad in (0, 32, 100, -64):
        with pytest.raises(ValueError):
            plan_variants(ref, [table[0][0]], checkpoint_every=bad)
    # a model without the cache path: everything from 0, no reference pass counted
    p4 = plan_variants(ref, [t[0] for t in table], checkpoint_every=E, max_batch_tokens=1 << 30, cached=False)
    assert set(p4.checkpoint.tolist()) == {0, -1} and p4.checkpoints == () and p4.tokens == 12 * 404


def test_single_substitutions():
    subs = single_substitutions("ACGT")
    assert len(subs) == 12 and subs[0] == (0, "C", "CCGT") and subs[-1] == (3, "G", "ACGG")
    assert single_substitutions("ACGT", positions=[2]) == [(2, "A", "ACAT"), (2, "C", "ACCT"), (2, "T", "ACTT")]
    with pytest.raises(ValueError):
        single_substitutions("ACGT", positions=[4])


# ------------------------------------------------------------------------------------------------ end to end on the oracle
class PrefixOracleOps(OracleOps):
    """OracleOps + the shared-prefix attention, by concatenation."""

    def __init__(self, act=torch.float64):
        super().__init__(act)
        self.prefix_calls = []

    def attention_prefix(self, q, k, v, k_pre, v_pre, vt_pre=None, prescaled=False):
        B, P = q.shape[0], k_pre.shape[0]
        self.prefix_calls.append((B, P, q.shape[1]))
        kc = torch.cat([k_pre.unsqueeze(0).expand(B, -1, -1, -1), k], dim=1)
        vc = torch.cat([v_pre.unsqueeze(0).expand(B, -1, -1, -1), v], dim=1)
        return self.attention(q, kc, vc, P)


@pytest.fixture(scope="module")
def small():
    from oracle.stripedhyena_ref import RefConfig, make_synthetic_state_dict
    from evo_amd.sh.model import StripedHyena
    sd = make_synthetic_state_dict(RefConfig.from_dict(SMALL), seed=3)
    m = StripedHyena(dict(SMALL), ops=PrefixOracleOps(torch.float64))
    m.load_state_dict({k: (v.double() if v.dtype == torch.bfloat16 else v) for k, v in sd.items()})
    return m


def _full_logprob_sum(model, seq):
    ids = torch.tensor([[TOK.eod_id] + list(seq.encode())])
    with torch.no_grad():
        lsm = torch.log_softmax(model(ids)[0][0, :-1].double(), -1)
    return float(lsm.gather(1, ids[0, 1:, None]).sum())


def test_score_variants_equals_full_forwards_on_the_oracle(small):
    rng = np.random.default_rng(5)
    ref = "".join(rng.choice(list("ACGT"), size=300))

    def sub(s, i):                                           # nucleotide index i = token index i + 1
        return s[:i] + ("A" if s[i] != "A" else "C") + s[i + 1:]
    variants = [sub(ref, 0), sub(ref, 63), sub(ref, 64), sub(ref, 130), sub(sub(ref, 140), 250), sub(ref, 299),
                ref[:150] + "GGA" + ref[150:], ref[:200] + ref[202:], ref[:280], ref]
    small.ops.prefix_calls.clear()
    res = score_variants(ref, variants, small, TOK, reduce_method="sum", checkpoint_every=64, device="cpu")
    ids = lambda s: [TOK.eod_id] + list(s.encode())          # noqa: E731
    plan = plan_variants(ids(ref), [ids(v) for v in variants], checkpoint_every=64)
    assert res.stats["tokens"] == plan.tokens < res.stats["naive_tokens"] == plan.naive_tokens
    assert res.stats["checkpoints"] == list(plan.checkpoints) and res.stats["passes"] == len(plan.groups) and res.stats["cached"]
    assert sorted(c for _, c, _ in small.ops.prefix_calls) == sorted(g.checkpoint for g in plan.groups if g.checkpoint > 0) != []
    assert np.array_equal(res.first_diff, plan.first_diff)
    ref_sum = _full_logprob_sum(small, ref)
    assert abs(res.reference_score - ref_sum) <= 1e-9 * 300
    for n, v in enumerate(variants):
        want = _full_logprob_sum(small, v)
        print(f"variant {n}: d = {res.first_diff[n]}, delta {res.delta[n]:.6f}, |delta - full| {abs(res.delta[n] - (want - ref_sum)):.2e}")
        assert abs(res.delta[n] - (want - ref_sum)) <= 1e-9 * (len(v) + len(ref))
        assert abs(res.score[n] - want) <= 1e-9 * len(v)
    assert res.delta[-1] == 0.0 and res.first_diff[-1] == -1
    # ... and the public scoring API (fp32 log-softmax on its host path)
    sums = score_sequences(variants + [ref], small, TOK, reduce_method="sum", device="cpu")
    for n, v in enumerate(variants):
        assert abs(res.delta[n] - (float(sums[n]) - float(sums[-1]))) <= 4e-4 * (len(v) + len(ref))
    mean = score_variants(ref, variants[:3], small, TOK, reduce_method="mean", checkpoint_every=64, device="cpu")
    assert np.allclose(mean.delta, res.delta[:3], rtol=0, atol=1e-9 * 600)
    assert np.allclose(mean.score, res.score[:3] / 300, rtol=0, atol=1e-9)


def test_reference_ending_right_behind_a_checkpoint_and_no_checkpoint_at_all(small):
    """(1) The reference is 129 tokens, a variant extends it by 200 nt: d = 129, c = 128, so the reference pass ends with a chunk of ONE
    token (a decode step of the cache path) and row 0 of the group has no target at all.  (2) Every change in front of the first
    checkpoint: no cached pass, the reference's log-probs come from row 0 of the stateless pass and no token is forwarded twice."""
    rng = np.random.default_rng(9)
    ref = "".join(rng.choice(list("ACGT"), size=128))
    variants = [ref + "".join(rng.choice(list("ACGT"), size=200)), ref[:100] + ("A" if ref[100] != "A" else "C") + ref[100:] + "ACGT" * 40]
    small.ops.prefix_calls.clear()
    res = score_variants(ref, variants, small, TOK, reduce_method="sum", checkpoint_every=64, device="cpu")
    assert res.first_diff.tolist() == [129, 101] and res.stats["checkpoints"] == [64, 128]
    assert sorted(small.ops.prefix_calls) == [(2, 64, 226), (2, 128, 201)]
    assert res.stats["tokens"] == 129 + 2 * 201 + 2 * 226
    ref_sum = _full_logprob_sum(small, ref)
    assert abs(res.reference_score - ref_sum) <= 1e-9 * 128
    for n, v in enumerate(variants):
        assert abs(res.delta[n] - (_full_logprob_sum(small, v) - ref_sum)) <= 1e-9 * (len(v) + len(ref))
    small.ops.prefix_calls.clear()
    early = [ref[:3] + ("A" if ref[3] != "A" else "C") + ref[4:], ref[:40], ref]
    res = score_variants(ref, early, small, TOK, reduce_method="sum", checkpoint_every=64, device="cpu")
    assert small.ops.prefix_calls == [] and res.stats["checkpoints"] == [] and res.stats["passes"] == 1 and res.stats["tokens"] == 3 * 129
    assert abs(res.reference_score - ref_sum) <= 1e-9 * 128 and res.delta[2] == 0.0
    for n, v in enumerate(early[:2]):
        assert abs(res.delta[n] - (_full_logprob_sum(small, v) - ref_sum)) <= 1e-9 * (len(v) + len(ref))
    only = score_variants(ref, [ref], small, TOK, reduce_method="sum", checkpoint_every=64, device="cpu")     # nothing but a copy
    assert only.stats["passes"] == 0 and only.stats["tokens"] == 129 and abs(only.reference_score - ref_sum) <= 1e-9 * 128


def test_other_model_objects_take_the_naive_path(small):
    class Plain:                                             # no hidden_states / ops: one full forward per batch
        def __call__(self, ids):
            return small(ids)
    ref = "ACGTTGCA" * 20
    variants = [ref[:5] + "T" + ref[6:], ref[:100], ref]
    res = score_variants(ref, variants, Plain(), TOK, reduce_method="sum", checkpoint_every=64, device="cpu")
    assert not res.stats["cached"] and res.stats["checkpoints"] == [] and res.stats["tokens"] == 3 * 161
    ref_sum = _full_logprob_sum(small, ref)
    for n, v in enumerate(variants):
        assert abs(res.delta[n] - (_full_logprob_sum(small, v) - ref_sum)) <= 1e-9 * (len(v) + len(ref))


# ------------------------------------------------------------------------------------------------ C ABI
def test_prefix_entries_are_exported_and_refuse_before_any_launch():
    header = open(os.path.join(ROOT, "include", "evo_mi355x.h")).read()
    for name in ("evo_attn_fwd_prefix_bf16", "evo_attn_prefix_vt_bf16"):
        assert name in _build.EXPORTS and name in evo_ops._SIGNATURES and re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert int(re.search(r"#define EVO_ABI_VERSION (\d+)", header).group(1)) == evo_ops.ABI_VERSION >= 14
    lib = evo_ops.load_library()
    one = ctypes.c_void_p(16)

    def call(P, Tq, row=None, q=one):
        row = max(P, 64) if row is None else row
        return lib.evo_attn_fwd_prefix_bf16(q, one, one, one, one, one, 1, 2, Tq, P, 768 * Tq, 768, 128, 768 * Tq, 768, 128, 768 * Tq, 768, 128,
                                            512, 128, row, 1.0, one, None)
    assert call(0, 200) == -1 and call(96, 200) == -1 and call(64, 128) == -1 and call(-64, 200) == -1
    assert call(128, 200, row=64) == -1 and call(128, 200, row=200) == -1 and call(64, 200, q=None) == -1
    assert lib.evo_attn_prefix_vt_bf16(one, one, 100, 2, 512, 128, 64, None) == -1      # plane narrower than its keys
    assert lib.evo_attn_prefix_vt_bf16(one, one, 100, 2, 512, 128, 136, None) == -1     # pitch not whole tiles
    assert lib.evo_attn_prefix_vt_bf16(one, one, 0, 2, 512, 128, 64, None) == -1


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_two_segment_attention_kernels_fit_their_budget():
    """The SEG instantiations of attn_fwd_w64_kernel, compiled with the flags the library is built with: no scratch, no VGPR spill,
    the LDS of the one-segment form (K ring 4 x 17,408 B + V^T ring 3 x 16,384 B)."""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-fno-gpu-rdc", "-Wno-inline-asm"] + _build.FILE_FLAGS["attn_w64.hip"] \
            + ["-S", "--cuda-device-only", os.path.join(ROOT, "evo_amd", "csrc", "attn_w64.hip"), "-o", out]
        proc = subprocess.run(cmd, capture_output=True, text=True)
        assert proc.returncode == 0, proc.stderr[-2000:]
        text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    seg = {}
    for blk in meta.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        if "attn_fwd_w64_kernel" in name and name.endswith("Lb1EEv8AttnArgs"):
            seg[name] = {k: int(re.search(r"\." + f + r":\s+(\d+)", blk).group(1)) for k, f in
                         (("spill", "vgpr_spill_count"), ("scratch", "private_segment_fixed_size"), ("lds", "group_segment_fixed_size"),
                          ("vgpr", "vgpr_count"))}
    assert len(seg) == 2, sorted(seg)                          # scores scaled in the kernel / queries pre-scaled
    for name, r in seg.items():
        assert r["spill"] == 0 and r["scratch"] == 0 and r["lds"] == W_LDS == 118784 and r["vgpr"] <= 512, (name, r)


# ------------------------------------------------------------------------------------------------ scripts/variants.py
def test_variants_cli_scan_on_the_oracle_backend(tmp_path, monkeypatch, small):
    """--scan --positions through evo_amd.Evo (stubbed to hand over the oracle-backend model, as tests/test_profile_host.py runs
    scripts/profile.py) reproduces the in-process numbers."""
    import types
    import evo_amd
    from scripts import variants as cli
    monkeypatch.setattr(evo_amd, "Evo", lambda name, device=None, weights=None: types.SimpleNamespace(model=small, tokenizer=TOK))
    ref = "".join(np.random.default_rng(8).choice(list("ACGT"), size=260))
    fa, tsv = tmp_path / "ref.fa", tmp_path / "out.tsv"
    fa.write_text(f">chrT some description\n{ref}\n")
    cli.main(["--reference", str(fa), "--scan", "--positions", "190-192", "--output-tsv", str(tsv), "--checkpoint-every", "64",
              "--reduce-method", "sum", "--weights", "synthetic", "--device", "cpu"])
    subs = single_substitutions(ref, range(190, 193))
    want = score_variants(ref, [s for _, _, s in subs], small, TOK, reduce_method="sum", checkpoint_every=64, device="cpu")
    lines = [l.split("\t") for l in open(tsv).read().splitlines()]
    assert lines[0] == ["name", "first_diff", "score", "delta"] and lines[1][0] == "#reference" and len(lines) == 2 + 9
    assert float(lines[1][2]) == want.reference_score
    for l, (p, alt, _), d, s, dl in zip(lines[2:], subs, want.first_diff, want.score, want.delta):
        assert l[0] == f"chrT:{ref[p]}{p}{alt}" and int(l[1]) == d == p + 1 and float(l[2]) == s and float(l[3]) == dl
    with pytest.raises(SystemExit):
        cli.main(["--reference", str(fa), "--scan", "--output-tsv", str(tsv), "--checkpoint-every", "100"])
    with pytest.raises(SystemExit):
        cli.main(["--reference", str(fa), "--output-tsv", str(tsv)])                    # neither --variants nor --scan
