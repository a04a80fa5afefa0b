"""CPU: the per-position profile layers that need no GPU -- the profile entry point of the C ABI (exported, host-side argument
checks), both instantiations of the fused tail's kernel body in the register / LDS budget (hipcc cross-compiles gfx950),
position_profiles / substitution_scores on the fp64 oracle backend, their argument checks, and scripts/profile.py end to end.

Tolerance of the API comparison: the fallback path (any model that is not the HIP engine) takes an FP32 log-softmax of the model's
logits, as score_sequences' host path does, so it is held against the fp64 log-softmax within the fp32 bound the suite already uses
for `logprob_entropy` (tests/test_gpu_kernels.py: 2e-5 x 20 = 4e-4 absolute), not within 1e-9."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import tempfile
import types

import numpy as np
import pytest
import torch

from evo_amd import _build
from evo_amd import ops as evo_ops
from evo_amd.tokenizer import CharLevelTokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
TOK = CharLevelTokenizer(512)
FP32_TOL = 2e-5 * 20


# ------------------------------------------------------------------------------------------------ C ABI
def test_profile_entry_point_is_exported_and_the_tables_agree():
    name = "evo_unembed_profile_bf16"
    assert name in _build.EXPORTS and name in evo_ops._SIGNATURES
    header = open(os.path.join(ROOT, "include", "evo_mi355x.h")).read()
    assert re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert int(re.search(r"#define EVO_ABI_VERSION (\d+)", header).group(1)) == evo_ops.ABI_VERSION >= 13
    lib = ctypes.CDLL(str(_build.build()))
    assert hasattr(lib, name)
    assert sorted(_build.EXPORTS) == sorted(evo_ops._SIGNATURES)


def _sel(*ids):
    return (ctypes.c_int32 * len(ids))(*ids)


def test_profile_argument_validation_needs_no_gpu():
    lib = evo_ops.load_library()
    p = ctypes.c_void_p(16)                 # (a non-null, 16-byte aligned pointer value: never dereferenced)
    f = lib.evo_unembed_profile_bf16
    # f(hidden, emb, target, sel, n_sel, sel_logprob, logprob, entropy, M, V, K, stream)
    ok = _sel(65, 67, 71, 84)
    assert f(p, p, None, ok, 4, p, None, None, 8, 256, 4096, None) == -1                 # V must be 512
    assert f(p, p, None, ok, 4, p, None, None, 8, 512, 100, None) == -1                  # K % 32
    assert f(p, p, None, ok, 0, p, None, None, 8, 512, 4096, None) == -1                 # n_sel < 1
    assert f(p, p, None, _sel(*range(9)), 9, p, None, None, 8, 512, 4096, None) == -1    # n_sel > 8
    assert f(p, p, None, None, 4, p, None, None, 8, 512, 4096, None) == -1               # NULL sel
    assert f(p, p, None, ok, 4, None, None, None, 8, 512, 4096, None) == -1              # NULL sel_logprob
    assert f(p, p, None, _sel(65, 512), 2, p, None, None, 8, 512, 4096, None) == -1      # id outside [0, 512)
    assert f(p, p, None, _sel(65, -1), 2, p, None, None, 8, 512, 4096, None) == -1
    assert f(p, p, None, _sel(65, 67, 65), 3, p, None, None, 8, 512, 4096, None) == -1   # an id twice
    assert f(p, p, None, ok, 4, p, None, None, 0, 512, 4096, None) == 0                  # legal, no rows: nothing launched


def test_binding_checks_the_ids_on_the_host():
    chk = evo_ops.HipOps.check_profile_ids
    assert chk([65, 67, 71, 84]) == [65, 67, 71, 84] and chk((511,)) == [511]
    for bad in ([], list(range(9)), [65, 65], [512], [-1], [1.5], "AC", None):
        with pytest.raises(ValueError):
            chk(bad)


# ------------------------------------------------------------------------------------------------ kernel resources
def _metadata(src):
    """{kernel name: {vgpr, spill, scratch, lds}} from the .amdgpu_metadata of `hipcc -S` (as tests/test_embed_host.py reads it)."""
    with tempfile.TemporaryDirectory() as td:
        out = os.path.join(td, "k.s")
        cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-gpu-rdc", "-Wno-inline-asm", "-S", "--cuda-device-only",
               os.path.join(ROOT, "evo_amd", "csrc", src), "-o", out]
        proc = subprocess.run(cmd, capture_output=True, text=True)
        assert proc.returncode == 0, proc.stderr[-2000:]
        text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    res = {}
    for blk in meta.split("  - .agpr_count:")[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk).group(1)
        res[name] = {"vgpr": int(re.search(r"\.vgpr_count:\s+(\d+)", blk).group(1)),
                     "spill": int(re.search(r"\.vgpr_spill_count:\s+(\d+)", blk).group(1)),
                     "scratch": int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1)),
                     "lds": int(re.search(r"\.group_segment_fixed_size:\s+(\d+)", blk).group(1))}
    return res


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_both_tail_instantiations_fit_two_workgroups_per_cu():
    kernels = _metadata("score_tail.hip")
    assert len(kernels) == 2, sorted(kernels)
    plain = [v for k, v in kernels.items() if "unembed_logprob_kernel" in k]
    prof = [v for k, v in kernels.items() if "unembed_profile_kernel" in k]
    assert len(plain) == 1 and len(prof) == 1, sorted(kernels)
    for name, r in kernels.items():
        assert r["spill"] == 0 and r["scratch"] == 0, (name, r)
        assert r["vgpr"] <= 256, (name, r)                      # two waves per SIMD = two workgroups per CU
        assert r["lds"] <= 80 * 1024, (name, r)                 # two workgroups in the CU's 160 KiB
    assert prof[0]["lds"] - plain[0]["lds"] == 64 * 8 * 4       # the parked logits of the selected columns: 2 KiB


# ------------------------------------------------------------------------------------------------ API on the fp64 oracle backend
LENGTHS = (1, 5, 33, 64)


@pytest.fixture(scope="module")
def small():
    """The SMALL config of tests/test_gpu_model.py with synthetic weights on the fp64 CPU oracle backend, a ragged ACGT batch, its
    profiles and the direct fp64 log-softmax of model(ids) per sequence (computed once, shared, never modified)."""
    from oracle.stripedhyena_ref import RefConfig, make_synthetic_state_dict
    from oracle_ops import OracleOps
    from test_gpu_model import SMALL
    from evo_amd.scoring import position_profiles
    from evo_amd.sh.model import StripedHyena
    sd = make_synthetic_state_dict(RefConfig.from_dict(SMALL), seed=3)
    m = StripedHyena(dict(SMALL), ops=OracleOps(torch.float64))
    m.load_state_dict({k: (v.double() if v.dtype == torch.bfloat16 else v) for k, v in sd.items()})
    rng = np.random.default_rng(11)
    seqs = ["".join(rng.choice(list("ACGT"), size=n)) for n in LENGTHS]
    profs = position_profiles(seqs, m, TOK, device="cpu")
    want = []
    with torch.no_grad():
        for s in seqs:
            ids = torch.tensor([[TOK.eod_id] + list(s.encode())])
            logits = m(ids)[0]
            assert logits.dtype == torch.float64
            want.append(torch.log_softmax(logits[0, :-1], -1).numpy())
    return types.SimpleNamespace(model=m, seqs=seqs, profs=profs, want=want)


def test_position_profiles_match_the_fp64_log_softmax(small):
    from evo_amd import PositionProfile
    assert [len(p.logprob) for p in small.profs] == list(LENGTHS)
    for s, p, w in zip(small.seqs, small.profs, small.want):
        L = len(s)
        assert isinstance(p, PositionProfile) and p.tokens == (65, 67, 71, 84)
        assert p.logprob.shape == (L,) and p.entropy.shape == (L,) and p.token_logprobs.shape == (L, 4)
        assert p.logprob.dtype == p.entropy.dtype == p.token_logprobs.dtype == np.float32
        obs = np.frombuffer(s.encode(), dtype=np.uint8).astype(np.int64)
        d_tok = np.abs(p.token_logprobs - w[:, [65, 67, 71, 84]]).max()
        d_lp = np.abs(p.logprob - w[np.arange(L), obs]).max()
        d_en = np.abs(p.entropy - (-(np.exp(w) * w).sum(-1))).max()
        print(f"L={L}: |token_logprobs - fp64| {d_tok:.2e}  |logprob - fp64| {d_lp:.2e}  |entropy - fp64| {d_en:.2e}")
        assert max(d_tok, d_lp, d_en) <= FP32_TOL                # (fp32 log-softmax in the fallback: module docstring)


def test_profiles_are_consistent_with_the_scoring_api(small):
    import evo_amd
    sums = evo_amd.score_sequences(small.seqs, small.model, TOK, reduce_method="sum", device="cpu")
    ents = evo_amd.positional_entropies(small.seqs, small.model, TOK, device="cpu")
    for s, p, tot, e in zip(small.seqs, small.profs, sums, ents):
        sub = evo_amd.substitution_scores(p)
        assert sub.shape == p.token_logprobs.shape
        for j, ch in enumerate("ACGT"):
            at = np.array([c == ch for c in s])
            assert np.array_equal(p.token_logprobs[at, j], p.logprob[at])      # the observed base's column IS the log-prob
            assert (sub[at, j] == 0.0).all()
        assert np.array_equal(sub, p.token_logprobs - p.logprob[:, None])
        assert np.sum(p.logprob) == tot                                          # what score_sequences(reduce_method="sum") sums
        assert np.array_equal(p.entropy, e)


def test_other_token_sets_and_helpers(small):
    from evo_amd.scoring import position_profiles, predicted_tokens, renormalized
    ids = [84, 0, 511, 65, 200, 71, 3, 67]
    profs = position_profiles(small.seqs[1:3], small.model, TOK, tokens=ids, device="cpu")
    for p, w, base in zip(profs, small.want[1:3], small.profs[1:3]):
        assert p.tokens == tuple(ids)
        assert np.abs(p.token_logprobs - w[:, ids]).max() <= FP32_TOL
        assert np.array_equal(p.token_logprobs[:, [3, 7, 5, 0]], base.token_logprobs)     # A, C, G, T columns of the default set
        assert np.array_equal(p.logprob, base.logprob)
    p = small.profs[2]
    assert np.array_equal(predicted_tokens(p), np.array([65, 67, 71, 84])[p.token_logprobs.argmax(-1)])
    r = renormalized(p)
    assert np.abs(np.exp(r.astype(np.float64)).sum(-1) - 1).max() < 1e-6
    assert np.array_equal(r.argmax(-1), p.token_logprobs.argmax(-1))
    one = position_profiles(small.seqs[:1], small.model, TOK, tokens="G", device="cpu")[0]
    assert one.token_logprobs.shape == (1, 1) and np.array_equal(one.token_logprobs[:, 0], small.profs[0].token_logprobs[:, 2])


class _NoDeviceModel:
    """Stands in for a model: any forward fails the test."""

    def hidden_states(self, *a, **k):
        raise AssertionError("device work started before the arguments were checked")

    __call__ = hidden_states


@pytest.mark.parametrize("tokens", ["", [], "ACGTNacgt", list(range(9)), "ACGA", [65, 67, 65], [512], [65, -1], "ACé", [1.5], 7])
def test_position_profiles_rejects_bad_tokens_before_device_work(tokens):
    from evo_amd import position_profiles
    with pytest.raises(ValueError):
        position_profiles(["ACGT"], _NoDeviceModel(), TOK, tokens=tokens, device="cpu")


# ------------------------------------------------------------------------------------------------ scripts/profile.py
def test_profile_cli_end_to_end_on_the_oracle_backend(tmp_path, monkeypatch, small):
    """FASTA in, .npz and long-form .tsv out, through evo_amd.Evo (stubbed to hand over the oracle-backend model, as
    tests/test_pool.py runs scripts/sample_many.py)."""
    import evo_amd
    from scripts import profile as cli
    monkeypatch.setattr(evo_amd, "Evo", lambda name, device=None, weights=None: types.SimpleNamespace(model=small.model, tokenizer=TOK))
    fa = tmp_path / "in.fa"
    recs = [("r0", small.seqs[2]), ("r1", small.seqs[0]), ("r2", small.seqs[1])]
    fa.write_text("".join(f">{n} some description\n{s}\n" for n, s in recs))
    npz, tsv = tmp_path / "out.npz", tmp_path / "out.tsv"
    cli.main(["--input-fasta", str(fa), "--output-npz", str(npz), "--output-tsv", str(tsv), "--tokens", "ACGT", "--batch-size", "2",
              "--weights", "synthetic", "--device", "cpu"])
    want = {"r0": small.profs[2], "r1": small.profs[0], "r2": small.profs[1]}
    z = np.load(npz)
    assert list(z["names"]) == ["r0", "r1", "r2"] and list(z["tokens"]) == [65, 67, 71, 84]
    assert sorted(z.files) == sorted(["names", "tokens"] + [f"{n}/{k}" for n in want for k in ("logprob", "entropy", "token_logprobs")])
    for n, p in want.items():
        # (a sequence scored in another batch: other padding, same rows -- the oracle backend is row-independent up to fp64 rounding)
        np.testing.assert_allclose(z[f"{n}/logprob"], p.logprob, rtol=0, atol=1e-6)
        np.testing.assert_allclose(z[f"{n}/entropy"], p.entropy, rtol=0, atol=1e-6)
        np.testing.assert_allclose(z[f"{n}/token_logprobs"], p.token_logprobs, rtol=0, atol=1e-6)
        assert z[f"{n}/token_logprobs"].dtype == np.float32
    lines = [l.split("\t") for l in open(tsv).read().splitlines()]
    assert lines[0] == ["name", "pos", "ref", "logprob", "entropy", "A", "C", "G", "T"]
    assert len(lines) == 1 + sum(len(s) for _, s in recs)
    row = 1
    for n, s in recs:
        for i, ch in enumerate(s):
            l = lines[row]
            assert l[:3] == [n, str(i), ch]
            assert np.float32(l[3]) == z[f"{n}/logprob"][i] and np.float32(l[4]) == z[f"{n}/entropy"][i]
            assert [np.float32(v) for v in l[5:]] == list(z[f"{n}/token_logprobs"][i])
            row += 1


def test_profile_cli_arguments():
    from scripts import profile as cli
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "profile.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--input-fasta", "--output-npz", "--output-tsv", "--tokens", "--batch-size", "--model-name", "--weights", "--device"):
        assert flag in r.stdout
    a = cli.build_parser().parse_args(["--input-fasta", "x.fa", "--output-tsv", "o.tsv"])
    assert a.tokens == "ACGT" and a.output_npz is None and a.device == "cuda:0"
    with pytest.raises(SystemExit):
        cli.main(["--input-fasta", "x.fa"])                                     # no output named
    with pytest.raises(SystemExit):
        cli.main(["--input-fasta", "x.fa", "--output-tsv", "o.tsv", "--tokens", "AAC"])      # a token twice: before any model is built
    assert cli.token_label(65) == "A" and cli.token_label(0) == "id0" and cli.token_label(511) == "id511"
