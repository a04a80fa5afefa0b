"""CPU: the sequence-embedding layers that need no GPU -- the pooling entry point of the C ABI (exported, host-side argument checks),
the pooling kernel's register budget (hipcc cross-compiles gfx950), embed_sequences' argument checks before any device work, and
scripts/embed.py's command line."""
import ctypes
import os
import re
import shutil
import subprocess
import sys
import tempfile

import pytest

from evo_amd import _build
from evo_amd import ops as evo_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_pool_entry_point_is_exported():
    assert "evo_pool_rows_bf16" in _build.EXPORTS and "evo_pool_rows_bf16" in evo_ops._SIGNATURES
    lib = ctypes.CDLL(str(_build.build()))
    assert hasattr(lib, "evo_pool_rows_bf16")


def test_pool_argument_validation_needs_no_gpu():
    lib = evo_ops.load_library()
    p = ctypes.c_void_p(16)                 # (a non-null, 16-byte aligned pointer value: never dereferenced)
    f = lib.evo_pool_rows_bf16
    # f(x, M, D, ld, ranges, B, scale, eps, mode, n_strips, ws, out, stream)
    assert f(None, 10, 256, 256, p, 1, None, 1e-6, 0, 1, p, p, None) == -1       # null x
    assert f(p, 10, 256, 256, None, 1, None, 1e-6, 0, 1, p, p, None) == -1       # null ranges
    assert f(p, 10, 256, 256, p, 1, None, 1e-6, 0, 1, None, p, None) == -1       # null workspace
    assert f(p, 10, 256, 256, p, 1, None, 1e-6, 0, 1, p, None, None) == -1       # null out
    assert f(p, 10, 100, 104, p, 1, None, 1e-6, 0, 1, p, p, None) == -1          # D % 8
    assert f(p, 10, 4104, 4104, p, 1, None, 1e-6, 0, 1, p, p, None) == -1        # D above the register plan (4096)
    assert f(p, 10, 256, 200, p, 1, None, 1e-6, 0, 1, p, p, None) == -1          # row pitch below D
    assert f(p, 10, 256, 256, p, 0, None, 1e-6, 0, 1, p, p, None) == -1          # B < 1
    assert f(p, 10, 256, 256, p, 1, None, 1e-6, 2, 1, p, p, None) == -1          # unknown mode
    assert f(p, 10, 256, 256, p, 1, None, 1e-6, -1, 1, p, p, None) == -1         # unknown mode
    assert f(p, 10, 256, 256, p, 1, None, 1e-6, 0, 0, p, p, None) == -1          # no strip


def _metadata(src):
    """{kernel name: {vgpr, spill, scratch}} from the .amdgpu_metadata of `hipcc -S` (as tests/test_kernel_resources.py reads it)."""
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
                     "scratch": int(re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk).group(1))}
    return res


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_pool_kernels_compile_without_spills():
    kernels = _metadata("pool.hip")
    strip = {k: v for k, v in kernels.items() if "pool_strip_kernel" in k}
    assert len(strip) == 8, sorted(kernels)                     # 4 register plans x (norm, plain)
    assert any("pool_finish_kernel" in k for k in kernels)
    for name, r in kernels.items():
        assert r["spill"] == 0 and r["scratch"] == 0, (name, r)
        assert r["vgpr"] <= 256, (name, r)                      # (at least two waves per SIMD)


class _NoDeviceModel:
    """Stands in for a model: any device work (embeddings / a forward) fails the test."""
    num_layers = 4

    def embeddings(self, *a, **k):
        raise AssertionError("device work started before the arguments were checked")

    __call__ = embeddings


@pytest.mark.parametrize("kw,msg", [
    (dict(layers=[4]), "outside"),
    (dict(layers=[-1]), "outside"),
    (dict(layers=["last"]), "block index"),
    (dict(layers=[]), "empty"),
    (dict(layers=[1, 1]), "twice"),
    (dict(layers=[1.5]), "block index"),
    (dict(pooling="max"), "pooling"),
])
def test_embed_sequences_rejects_bad_arguments_before_device_work(kw, msg):
    from evo_amd import embed_sequences
    from evo_amd.tokenizer import CharLevelTokenizer
    with pytest.raises(ValueError, match=msg):
        embed_sequences(["ACGT"], _NoDeviceModel(), CharLevelTokenizer(512), device="cpu", **kw)


def test_embed_sequences_rejects_empty_input():
    from evo_amd import embed_sequences
    from evo_amd.tokenizer import CharLevelTokenizer
    with pytest.raises(ValueError, match="no sequences"):
        embed_sequences([], _NoDeviceModel(), CharLevelTokenizer(512), device="cpu")
    with pytest.raises(ValueError, match="empty sequence"):
        embed_sequences(["ACGT", ""], _NoDeviceModel(), CharLevelTokenizer(512), device="cpu")


def test_layers_accept_the_cli_form():
    from evo_amd.embeddings import normalize_layers
    assert normalize_layers("16,final", 32) == [16, "final"]
    assert normalize_layers(("final", 0, 31), 32) == ["final", 0, 31]


def test_embed_cli_help_runs():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "embed.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    for flag in ("--input-fasta", "--output-npz", "--model-name", "--weights", "--device", "--batch-size", "--layers", "--pooling"):
        assert flag in r.stdout


def test_model_embeddings_refuses_what_it_does_not_support():
    import torch
    from evo_amd.sh.model import StripedHyena
    m = StripedHyena(dict(vocab_size=512, hidden_size=256, num_layers=4, attn_layer_idxs=[2], num_attention_heads=2))
    ids = torch.zeros(1, 8, dtype=torch.long)
    with pytest.raises(ValueError, match="padding_mask"):
        m.embeddings(ids, ["final"], padding_mask=torch.ones(1, 8))
    with pytest.raises(ValueError, match="cache"):
        m.embeddings(ids, ["final"], inference_params_dict={})
    with pytest.raises(RuntimeError, match="GPU"):                  # weights on the host
        m.embeddings(ids, ["final"])
    assert m.has_own_unembed and hasattr(m.unembed, "unembed")
