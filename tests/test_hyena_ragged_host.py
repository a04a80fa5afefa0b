"""CPU: the C entry of the ragged Hyena end state (evo_hyena_state_at_zt, csrc/hyena_ragged.hip) -- what needs no GPU.

  * exported, declared, bound; the header's ABI version is the binding's and at least 16; the segment length is one constant;
  * every contract violation of include/evo_mi355x.h returns -1 before any launch (null or never-dereferenced pointers), and the
    workspace query (ws == NULL) answers with the bytes the launches need;
  * resources: both kernels compile for gfx950 without scratch."""
import ctypes
import os
import re

import pytest

from evo_amd import _build
from evo_amd import ops as evo_ops
from test_kernel_resources import HIPCC, _metadata

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "evo_hyena_state_at_zt"


def test_entry_is_exported_declared_and_bound():
    header = open(os.path.join(ROOT, "include", "evo_mi355x.h")).read()
    assert NAME in _build.EXPORTS and NAME in evo_ops._SIGNATURES and re.search(r"\bint\s+" + NAME + r"\s*\(", header)
    assert int(re.search(r"#define EVO_ABI_VERSION (\d+)", header).group(1)) == evo_ops.ABI_VERSION >= 16
    assert int(re.search(r"#define EVO_HYENA_RAGGED_SEG (\d+)", header).group(1)) == evo_ops.HYENA_RAGGED_SEG
    assert evo_ops.HYENA_RAGGED_SEG % 8 == 0
    # the citation `s_out` of evo_hyena_ct carries
    decl = header[:header.index("int " + NAME)]
    assert "[REF evo/generation.py:111-117,152]" in decl[decl.rindex("/* ----"):]
    lib = evo_ops.load_library()
    assert lib.evo_abi_version() == evo_ops.ABI_VERSION and hasattr(lib, NAME)
    assert hasattr(evo_ops.HipOps, "hyena_state_at_zt") and hasattr(evo_ops.HipOps, "hyena_state_at")


def test_contract_violations_are_refused_before_any_launch():
    lib = evo_ops.load_library()
    one = ctypes.c_void_p(16)                                            # non-null, aligned, never dereferenced
    SEG = evo_ops.HYENA_RAGGED_SEG

    def call(**kw):
        a = dict(zt=one, lens=one, fir_w=one, fir_b=one, poles=one, s_out=one, fir_out=one, ws=one, ws_bytes=1 << 40, B=3, T=320, D=256,
                 H=2, zt_pitch=1024, row_pitch=320, zt_row0=0)
        a.update(kw)
        return lib.evo_hyena_state_at_zt(a["zt"], a["lens"], a["fir_w"], a["fir_b"], a["poles"], a["s_out"], a["fir_out"], a["ws"],
                                         a["ws_bytes"], a["B"], a["T"], a["D"], a["H"], a["zt_pitch"], a["row_pitch"], a["zt_row0"], None)

    def need(B, T, D):
        return B * -(-T // SEG) * D * 8 * 8                              # a c64 per (row, segment, channel, mode)

    # the workspace query: nothing launched, the bytes returned; one byte short is refused
    assert call(ws=None, ws_bytes=0) == need(3, 320, 256)
    assert call(ws=None, ws_bytes=0, B=1, T=131072, D=128, H=1, zt_pitch=131072, row_pitch=131072) == need(1, 131072, 128)
    assert call(ws_bytes=need(3, 320, 256) - 1) == -1 and call(ws_bytes=0) == -1
    assert call(ws=ctypes.c_void_p(8)) == -1                             # a workspace that is not 16-byte aligned
    for name in ("zt", "lens", "fir_w", "fir_b", "poles", "s_out", "fir_out"):
        assert call(**{name: None}) == -1, name                          # null pointers -- also in a query
        assert call(**{name: None}, ws=None) == -1, name
    assert call(zt=ctypes.c_void_p(8)) == -1                             # z^T is read 16 bytes at a time
    for name in ("B", "T", "D", "H"):
        assert call(**{name: 0}) == -1 and call(**{name: -1}) == -1, name
    assert call(D=256, H=1) == -1 and call(D=192, H=2) == -1 and call(D=384, H=2) == -1      # D == n_heads * 128
    assert call(T=300, row_pitch=304) == -1                              # T % 64 != 0 with more than one row ...
    assert call(B=1, T=300, row_pitch=304, ws=None) == need(1, 300, 256)                    # ... is the B = 1 form
    assert call(row_pitch=324) == -1 and call(row_pitch=316) == -1      # % 8, and rows that overlap
    assert call(row_pitch=256) == -1
    assert call(zt_row0=4) == -1 and call(zt_row0=-8) == -1
    assert call(zt_pitch=1000) == -1 and call(zt_pitch=0) == -1 and call(zt_pitch=768) == -1       # % 256; 3 rows of 320 need 960 positions
    assert call(zt_row0=128, zt_pitch=1024) == -1 and call(zt_row0=128, zt_pitch=1280, ws=None) > 0
    assert call(B=256, T=8192, D=4096, H=32, row_pitch=8192, zt_pitch=256 * 8192) == -1        # a workspace beyond 2 GiB has no answer in an int
    assert call(ws=None) > 0                                             # and the arguments above are otherwise fine


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_ragged_state_kernels_need_no_scratch():
    meta = _metadata("hyena_ragged.hip")
    for pattern, max_vgpr in (("hyena_ragged_partial_kernel", 128), ("hyena_ragged_combine_kernel", 64)):
        ks = {k: v for k, v in meta.items() if pattern in k}
        assert len(ks) == 1, sorted(meta)
        for name, r in ks.items():
            print(name, r)
            assert r["scratch"] == 0 and r["vgpr"] <= max_vgpr and r["lds"] == 0, (name, r)
