"""CPU: the C-ABI shared library builds, loads, and exports every symbol include/evo_mi355x.h declares;
the ctypes table in evo_amd/ops.py covers exactly that set; the product path refuses to run without a GPU
instead of falling back."""
import ctypes
import os
import re

import pytest
import torch

from evo_amd import _build
from evo_amd import ops as evo_ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    text = open(os.path.join(ROOT, "include", "evo_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\bint\s+(evo_\w+)\s*\(", text)))


def test_header_table_and_exports_agree():
    declared = _declared()
    assert declared, "no declarations parsed"
    assert sorted(_build.EXPORTS) == declared
    assert sorted(evo_ops._SIGNATURES) == declared


def test_library_builds_and_exports_every_symbol():
    path = _build.build()
    lib = ctypes.CDLL(str(path))
    for name in _declared():
        assert hasattr(lib, name), name
    lib.evo_abi_version.restype = ctypes.c_int
    assert lib.evo_abi_version() == evo_ops.ABI_VERSION == int(re.search(r"#define EVO_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "evo_mi355x.h")).read()).group(1))
    assert evo_ops.load_library() is not None


def test_argument_validation_needs_no_gpu():
    lib = evo_ops.load_library()
    # bad shapes are rejected on the host before any launch
    assert lib.evo_rmsnorm_bf16(None, None, None, None, 4, 7, 1e-6, None) == -1
    assert lib.evo_hyena_apply(None, None, None, None, None, None, None, None, None, None, 1, 16, 256, 3, 64, None) == -1
    assert lib.evo_hyena_apply(None, None, None, None, None, None, None, None, None, None, 1, 16, 256, 2, 6, None) == -1
    assert lib.evo_hyena_seg_state(None, None, None, None, None, None, None, 1, 16, 256, 2, 6, None) == -1
    assert lib.evo_embed_bf16(None, None, None, 4, 12, 512, None, None) == -1          # D not a multiple of 8
    assert lib.evo_embed_bf16(None, None, None, 4, 16, 0, None, None) == -1            # empty vocabulary
    assert lib.evo_unembed_logprob_bf16(None, None, None, None, None, 8, 256, 4096, None) == -1    # V must be 512
    assert lib.evo_unembed_logprob_bf16(None, None, None, None, None, 8, 512, 100, None) == -1     # K % 32
    assert lib.evo_linear_mfma_bf16(None, None, None, None, None, 16, 256, 96, None) == -1           # K % 64
    assert lib.evo_linear_mfma_bf16(None, None, None, None, None, 16, 100, 64, None) == -1           # N % 256
    assert lib.evo_gelu_gate_bf16(None, None, 4, 12, None) == -1
    assert lib.evo_mlp_gate_mfma_bf16(None, None, None, 256, 100, 128, None) == -1                   # (2 I) % 256
    assert lib.evo_mlp_gate_mfma_bf16(None, None, None, 256, 128, 96, None) == -1                    # K % 64
    one = ctypes.c_void_p(16)                                                                       # (a non-null, 16-byte aligned pointer value: never dereferenced)
    # evo_hyena_ct(..., B, T, D, H, zt_pitch, row_pitch, zt_row0, tail_T, tail_pos0, state_only, y_blocked_rows, y_row0, y_row_pitch, stream)
    assert lib.evo_hyena_ct(one, None, None, None, None, one, None, None, None, 2, 100, 256, 2, 256, 100, 0, 0, 0, 0, 0, 0, 0, None) == -1   # row pitch % 8
    assert lib.evo_hyena_ct(one, None, None, None, None, one, None, None, None, 2, 100, 256, 2, 200, 104, 0, 0, 0, 0, 0, 0, 0, None) == -1   # z^T not whole 256-position blocks
    assert lib.evo_hyena_ct(one, None, None, None, None, one, None, None, None, 3, 100, 256, 2, 256, 104, 0, 0, 0, 0, 0, 0, 0, None) == -1   # rows beyond z^T
    assert lib.evo_hyena_ct(one, None, None, None, None, one, None, None, None, 2, 100, 256, 2, 256, 104, 4, 0, 0, 0, 0, 0, 0, None) == -1   # first position % 8
    assert lib.evo_hyena_ct(one, None, None, None, None, None, None, None, None, 2, 100, 256, 2, 256, 104, 0, 0, 0, 1, 0, 0, 0, None) == -1  # state-only without s_out
    assert lib.evo_hyena_ct(one, None, None, None, None, one, None, None, None, 2, 513, 256, 2, 1280, 512, 0, 500, 1024, 0, 0, 0, 0, None) == -1   # tail_T % 512
    assert lib.evo_hyena_ct(one, None, None, None, None, one, None, None, None, 2, 530, 256, 2, 1280, 512, 0, 512, 1024, 0, 0, 0, 0, None) == -1   # more than 8 tail tokens
    assert lib.evo_hyena_ct(one, None, None, None, None, one, None, None, None, 2, 513, 256, 2, 1280, 512, 0, 512, 1000, 0, 0, 0, 0, None) == -1   # tail block inside the main area
    assert lib.evo_hyena_ct(one, None, None, None, None, one, None, None, None, 2, 104, 256, 2, 256, 104, 0, 0, 0, 0, 0, 0, 100, None) == -1   # y_row_pitch below T
    assert lib.evo_linear_t_mfma_bf16(None, None, None, None, 300, 768, 256, None) == -1              # Mp % 256
    assert lib.evo_linear_t_mfma_bf16(None, None, None, None, 512, 700, 256, None) == -1              # N % 256
    assert lib.evo_rmsnorm_rows_bf16(None, None, None, None, 200, 64, 1e-6, 100, 96, 100, 0, None) == -1      # pitch < Tm
    assert lib.evo_rmsnorm_rows_bf16(None, None, None, None, 250, 64, 1e-6, 100, 104, 100, 0, None) == -1     # M % T
    assert lib.evo_rmsnorm_rows_bf16(None, None, None, None, 200, 64, 1e-6, 100, 96, 96, 100, None) == -1     # tail rows inside the main rows
    lib.evo_rope_append_decode_bf16.restype = ctypes.c_int
    assert lib.evo_rope_append_decode_bf16(None, None, None, None, ctypes.c_float(1.0), 1, 32, 128, 8, 8, 8, 8, ctypes.c_float(1.0), None) == -1   # null tensors
    assert lib.evo_attn_fwd_causal_bf16(None, None, None, None, 1, 1, 4, 4, -1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1.0, None, None) == -1


def test_fp8_decode_attention_refuses_one_stride_step_beyond_its_largest_offset():
    """evo_attn_decode_fp8 addresses a key by a 32-bit byte offset: at Tk = 2,100 the largest token stride it admits is 2,045,216 bytes
    (tests/test_gpu_kv_fp8_exact.py launches there); one 16-byte step further, Tk * d_st = 4,294,987,200 >= 2^32 - 1, is refused with -1
    before any launch (the pointers are never dereferenced)."""
    from kv_fp8_exact import BIG_TK, largest_token_stride
    lib = evo_ops.load_library()
    one = ctypes.c_void_p(16)
    st = largest_token_stride()
    assert BIG_TK * st <= 0xffffffff - 1 < BIG_TK * (st + 16)

    def call(Tk, d_st):
        return lib.evo_attn_decode_fp8(one, one, one, one, 2, 2, Tk, 768, 128, 512, d_st, 256, 128, 4 * Tk, 2 * Tk, Tk, None, one, one, 1,
                                       ctypes.c_float(0.0), None)
    assert call(BIG_TK, st + 16) == -1
    assert call(BIG_TK + 1, st) == -1                                  # the same stride, one key more
    assert call(BIG_TK, st + 8) == -1                                  # (not a multiple of 16)


def test_c_abi_reads_no_environment():
    """Which kernel a C-ABI call launches is a function of its arguments alone (no global state inside the boundary): no
    source or header of the library mentions getenv."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "evo_amd", "csrc", "*")) + glob.glob(os.path.join(ROOT, "include", "*")))
    assert any(f.endswith(".hip") for f in files) and any(f.endswith(".h") for f in files)
    assert [os.path.relpath(f, ROOT) for f in files if "getenv" in open(f, errors="replace").read()] == []


def test_binding_refuses_misaligned_addresses():
    """include/evo_mi355x.h, Conventions: bf16 / f32 / c64 data 16-byte aligned and no more, integer vectors at their element's alignment.  HipOps._need, the attention launches' operand check
    (_need_strided) and the hand-rolled checks of attention_decode / rope_append_decode / pool_rows go through this one helper, which takes an address: no GPU needed."""
    chk = evo_ops.HipOps._check_address
    for addr in (0, 16, 0x7f0000000010, 0x7f0000000200, 48):                                    # 16 (mod 32) is legal: nothing more is asked
        chk(addr, "x")
    for addr in (8, 2, 0x7f0000000008, 0x7f0000000204, 17):
        with pytest.raises(RuntimeError, match="not 16-byte aligned"):
            chk(addr, "x")
    with pytest.raises(RuntimeError, match="rmsnorm x: address 0x40 is not 128-byte aligned"):
        chk(64, "rmsnorm x", align=128)
    assert evo_ops.HipOps.PTR_ALIGN == 16
    al = evo_ops.HipOps._align_of                                                                # floating-point data: 16; integer vectors: the element
    assert [al(d) for d in (torch.bfloat16, torch.float32, torch.complex64, torch.int64, torch.int32, torch.uint8)] == [16, 16, 16, 8, 4, 1]
    import inspect
    for name in ("_need", "_need_strided", "attention_decode", "rope_append_decode", "pool_rows"):   # the check is wired into every place the issue names
        assert "_check_address(" in inspect.getsource(getattr(evo_ops.HipOps, name)), name
    for name in ("attention", "attention_prefix", "attention_decode", "attention_decode_prefix"):   # (their q / k / v operands: one helper)
        assert "self._need_strided(" in inspect.getsource(getattr(evo_ops.HipOps, name)), name


@pytest.mark.skipif(torch.cuda.is_available(), reason="CPU-only behaviour")
def test_no_cpu_fallback():
    from evo_amd.sh.model import StripedHyena
    with pytest.raises(evo_ops.EvoLibraryError):
        evo_ops.HipOps()
    m = StripedHyena(dict(hidden_size=128, num_layers=1, attn_layer_idxs=[], num_attention_heads=1))
    with pytest.raises(evo_ops.EvoLibraryError):
        m(torch.zeros(1, 4, dtype=torch.long))


def test_pack_gate_weights_layout():
    """HipOps.pack_gate_weights: the row order evo_mlp_gate_mfma_bf16 documents in include/evo_mi355x.h -- blocks of 64 rows =
    rows 32 q .. 32 q + 31 of W1 followed by the same rows of W2 (pure host logic, no GPU)."""
    import torch
    I, K = 96, 8
    w12 = torch.arange(2 * I * K, dtype=torch.float32).view(2 * I, K)
    g = evo_ops.HipOps.pack_gate_weights(w12)
    assert g.shape == w12.shape and g.is_contiguous()
    for q in range(I // 32):
        assert torch.equal(g[64 * q: 64 * q + 32], w12[32 * q: 32 * q + 32])                 # W1 rows
        assert torch.equal(g[64 * q + 32: 64 * q + 64], w12[I + 32 * q: I + 32 * q + 32])     # the same rows of W2
    import pytest
    with pytest.raises(ValueError):
        evo_ops.HipOps.pack_gate_weights(torch.zeros(2 * 40, K))                             # inner size not a multiple of 32
