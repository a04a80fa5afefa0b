"""CPU: FP8 (e4m3fn) weights of the decode step at 9-64 rows (csrc/skinny_fp8.hip) -- what can be held without a GPU.

  1. the two entries are exported, declared in the header and bound with matching signatures; the ABI is still 20;
  2. both refuse null / misaligned pointers and bad shapes with -1 before any launch (no GPU here: a launch would fail differently);
  3. the row limit is the BACKEND's (Backend.W8_ROWS): on a subclass of the fp64 oracle backend that declares 64 rows a 12-slot pool and
     a 9-prompt generate() equal the model holding the dequantised weights bit for bit; 65 rows and a layer whose K is no multiple of 256
     are refused before any backend call, the latter from 9 rows on only;
  4. the compiler's metadata of csrc/skinny_fp8.hip: no scratch, no spills;
  5. the four-bit design's 24-bit bound (tests/w8_ref.py) at every K of tests/test_gpu_w8_wide.py, and the slice rule replayed.
"""
import ctypes
import os
import re
import shutil
import subprocess
import tempfile

import pytest
import torch

import dense_exact as DX
import w8_ref as W8
import w8_wide_ref as WW
from evo_amd import _build
from evo_amd import ops as evo_ops
from evo_amd.backend import Backend
from evo_amd.generation import Generator, generate
from evo_amd.pool import DecodePool, sample_many
from evo_amd.sh.cache import Fp8Weight, check_weight_rows
from test_fanout_host import SMALL, TOK
from test_w8_host import STREAMED, _model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("evo_linear_skinny_w8", "evo_mlp_gate_skinny_w8")
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


# ------------------------------------------------------------------------------------------------ 1. wiring
def test_entries_are_wired():
    header = open(os.path.join(ROOT, "include", "evo_mi355x.h")).read()
    lib = evo_ops.load_library()
    for name in ENTRIES:
        assert name in _build.EXPORTS and name in evo_ops._SIGNATURES and hasattr(lib, name), name
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header, re.S)
        assert decl, name
        assert len([a for a in decl.group(1).split(",") if a.strip()]) == len(evo_ops._SIGNATURES[name][0]), name
    assert int(re.search(r"#define EVO_ABI_VERSION (\d+)", header).group(1)) == evo_ops.ABI_VERSION == 20
    assert lib.evo_abi_version() == 20
    assert evo_ops._SIGNATURES["evo_linear_skinny_w8"] == evo_ops._SIGNATURES["evo_linear_small_m_w8"]       # the sibling's arguments
    assert evo_ops._SIGNATURES["evo_mlp_gate_skinny_w8"] == evo_ops._SIGNATURES["evo_mlp_gate_small_m_w8"]
    assert any(p.name == "skinny_fp8.hip" for p in _build.sources())
    assert Backend.W8_ROWS == 8 and evo_ops.HipOps.W8_ROWS == 64 and W8.W8OracleOps.W8_ROWS == 8


# ------------------------------------------------------------------------------------------------ 2. refusals of the entries
ONE = ctypes.c_void_p(16)                                             # non-null, 16-byte aligned, never dereferenced
BAD_SHAPES = [dict(M=0), dict(M=4), dict(M=65), dict(M=-1), dict(K=0), dict(K=128), dict(K=4104), dict(K=-256)]


def _caller(name, ok):
    f, names = getattr(evo_ops.load_library(), name), list(ok)
    assert len(evo_ops._SIGNATURES[name][0]) == len(names)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return f(*[a[n] for n in names])
    return call


def _refuses(call, required, optional, sizes, scale_name):
    for n in required:
        assert call(**{n: None}) == -1, n
        assert call(**{n: ctypes.c_void_p(18) if n == scale_name else ctypes.c_void_p(8)}) == -1, n
    for n in optional:
        assert call(**{n: ctypes.c_void_p(8)}) == -1, n
    for kw in list(sizes) + BAD_SHAPES:
        assert call(**kw) == -1, kw


def test_entries_refuse_before_any_launch():
    ok = dict(x=ONE, w_data=ONE, w_scale=ONE, bias=ONE, residual=ONE, y=ONE, M=9, N=64, K=256, ws=None, ws_bytes=0, stream=None)
    _refuses(_caller("evo_linear_skinny_w8", ok), ("x", "w_data", "w_scale", "y"), ("bias", "residual", "ws"),
             [dict(N=0), dict(N=-4), dict(N=2 ** 31), dict(K=2 ** 31), dict(ws=ctypes.c_void_p(24), ws_bytes=1 << 20), dict(ws=ONE, ws_bytes=-1)],
             "w_scale")
    ok = dict(x=ONE, w12_data=ONE, w12_scale=ONE, a=ONE, M=9, I=64, K=256, grouped=0, stream=None)
    _refuses(_caller("evo_mlp_gate_skinny_w8", ok), ("x", "w12_data", "w12_scale", "a"), (),
             [dict(I=0), dict(I=40), dict(I=40, grouped=1), dict(I=-32), dict(I=2 ** 30)], "w12_scale")


# ------------------------------------------------------------------------------------------------ 3. the limit is the backend's
class WideOracleOps(W8.W8OracleOps):
    """The fp64 oracle backend declaring the wide rows; counts every kernel-level call a refusal must precede."""
    W8_ROWS = 64

    def __init__(self):
        super().__init__(torch.float64)
        self.calls = 0

    def embed(self, *a, **kw):
        self.calls += 1
        return super().embed(*a, **kw)

    def w_quant_fp8(self, w):
        self.calls += 1
        return super().w_quant_fp8(w)


WIDE_OK = dict(SMALL, inner_mlp_size=768)                             # every streamed K a multiple of 256 (D = 256, l3: 768)
TWELVE = ["ACGTTGCA", "GGATTACA", "TTTTACGA", "CATGCATG", "AAAACCCC", "GTGTGTGT", "TACGTACG", "CCGGAATT", "AGAGAGTC", "TTGACAGG", "ACACACAC",
          "GATTACAG"]


def _twin_of(m, cfg):
    """The same model with every streamed weight replaced by its dequantised value, in bf16 format."""
    twin = _model(WideOracleOps(), cfg=cfg)
    twin.load_state_dict({k: (Fp8Weight.quantize(v).dequantize(torch.bfloat16).double() if k.endswith(STREAMED) else v.clone())
                          for k, v in m.state_dict().items()})
    return twin


def test_check_weight_rows_takes_the_backends_figure():
    check_weight_rows(8, "n_slots")
    check_weight_rows(64, "n_slots", 64)
    with pytest.raises(ValueError) as e8:
        check_weight_rows(9, "n_slots")
    assert str(e8.value) == ('weight_dtype="fp8" serves at most 8 rows per decode step, got n_slots = 9 (the 9-64-row launches are bf16 only)')
    with pytest.raises(ValueError, match="at most 64 rows per decode step, got n_slots = 65$"):
        check_weight_rows(65, "n_slots", 64)


def test_a_backend_that_declares_64_rows_runs_12_slots_and_9_prompts():
    m = _model(WideOracleOps(), cfg=WIDE_OK)
    twin = _twin_of(m, WIDE_OK)
    kw = dict(n_slots=12, top_k=1, top_p=1.0, temperature=0.0, device="cpu")
    p8 = DecodePool(twin, TOK, weight_dtype="fp8", **kw)
    s8, sc8, o8 = p8.generate(TWELVE, n_tokens=6, n_sample_per_prompt=1)
    assert twin.ops.w8_calls["gate"] == p8.stats["steps"] * twin.num_layers > 0
    pd = DecodePool(twin, TOK, **kw)
    sd, scd, od = pd.generate(TWELVE, n_tokens=6, n_sample_per_prompt=1)
    assert s8 == sd and o8 == od and sc8 == scd and len(s8) == 12
    assert torch.equal(p8.last_ids, pd.last_ids) and torch.equal(p8.last_logits, pd.last_logits)
    assert p8.stats["weight_dtype"] == "fp8" and p8.stats["decode_weight_bytes"] == twin.decode_weight_bytes("fp8")
    # on the original weights the FP8 steps run too, and differ from the bf16 ones (the format is not a no-op)
    po = DecodePool(m, TOK, weight_dtype="fp8", **kw)
    po.generate(TWELVE, n_tokens=6, n_sample_per_prompt=1)
    pb = DecodePool(m, TOK, **kw)
    pb.generate(TWELVE, n_tokens=6, n_sample_per_prompt=1)
    assert m.ops.w8_calls["gate"] > 0 and not torch.equal(po.last_logits, pb.last_logits)
    # generate() with 9 prompts, and Generator on a batch of 9
    g8, _ = generate(TWELVE[:9], twin, TOK, n_tokens=4, cached_generation=True, device="cpu", verbose=0, weight_dtype="fp8", top_k=1)
    gd, _ = generate(TWELVE[:9], twin, TOK, n_tokens=4, cached_generation=True, device="cpu", verbose=0, top_k=1)
    assert g8 == gd and len(g8) == 9
    ids = torch.tensor([list(p.encode()) for p in TWELVE[:9]])
    out = {}
    for fmt in ("fp8", "bf16"):
        out[fmt] = Generator(twin, TOK, top_k=1, top_p=1.0, temperature=0.0, weight_dtype=fmt).generate(
            "cpu", input_ids=ids, num_tokens=6, cached_generation=True, print_generation=False, stop_at_eos=False)
    assert torch.equal(out["fp8"][0], out["bf16"][0]) and torch.equal(out["fp8"][1], out["bf16"][1])
    _, seqs, _ = sample_many(TWELVE[:9], twin, TOK, n_tokens=3, temp=0.0, top_k=1, n_slots=9, device="cpu", weight_dtype="fp8")
    assert seqs == [x[:3] for x in s8[:9]]


def test_beam_search_on_a_12_slot_fp8_pool():
    """beam_search on an FP8 pool of more than 8 slots runs FP8 steps (section 22's composition, at the wide rows)."""
    from beam_ref import BeamOracleOps

    class BeamWideOps(WideOracleOps, BeamOracleOps):
        pass
    m = _model(BeamWideOps(), cfg=WIDE_OK)
    pool = DecodePool(m, TOK, n_slots=12, device="cpu", share_prompt_kv=True, weight_dtype="fp8")
    res = pool.beam_search(TWELVE[:3], 3, beam_width=4)
    L, steps = m.num_layers, pool.stats["beam_steps"]
    assert len(res) == 3 and steps > 0
    assert m.ops.w8_calls["gate"] == steps * L and m.ops.w8_calls["linear"] == 2 * steps * L
    with pytest.raises(ValueError, match="batch_invariant"):
        DecodePool(m, TOK, n_slots=12, device="cpu", weight_dtype="fp8", batch_invariant=True)


def test_wide_refusals_come_before_any_backend_call():
    m = _model(WideOracleOps(), cfg=WIDE_OK)
    with pytest.raises(ValueError, match="at most 64"):
        DecodePool(m, TOK, n_slots=65, device="cpu", weight_dtype="fp8")
    with pytest.raises(ValueError, match="at most 64"):
        generate(["ACGTACGT"] * 65, m, TOK, n_tokens=2, cached_generation=True, device="cpu", verbose=0, weight_dtype="fp8")
    with pytest.raises(ValueError, match="at most 64"):
        Generator(m, TOK, weight_dtype="fp8").generate("cpu", input_ids=torch.zeros(65, 4, dtype=torch.long), num_tokens=2)
    DecodePool(m, TOK, n_slots=64, device="cpu", weight_dtype="fp8")
    # l3's K = 688 (SMALL's padded inner size): a multiple of 16, not of 256 -- refused from 9 rows on, by name
    odd = _model(WideOracleOps(), cfg=SMALL)
    assert odd._padded_inner() % 256 and odd._padded_inner() % 16 == 0
    for make in (lambda: DecodePool(odd, TOK, n_slots=9, device="cpu", weight_dtype="fp8"),
                 lambda: generate(["ACGTACGT"] * 9, odd, TOK, n_tokens=2, cached_generation=True, device="cpu", verbose=0, weight_dtype="fp8"),
                 lambda: Generator(odd, TOK, weight_dtype="fp8").generate("cpu", input_ids=torch.zeros(9, 4, dtype=torch.long), num_tokens=2),
                 lambda: odd.check_fp8_weights(9)):
        with pytest.raises(ValueError, match=r"blocks\.0\.mlp\.l3 has K = 688, not a multiple of 256"):
            make()
    DecodePool(odd, TOK, n_slots=8, device="cpu", weight_dtype="fp8")
    Generator(odd, TOK, weight_dtype="fp8")
    odd.check_fp8_weights(8)
    # the step itself refuses too (a cache whose flag was set by hand), before any FP8 call
    ipd = odd.initialize_inference_params()
    ipd["mha"].max_batch_size = ipd["hyena"].max_batch_size = 9
    with torch.inference_mode():
        _, ipd = odd(torch.tensor([[65, 67, 71]] * 9), inference_params_dict=ipd)
        calls = dict(odd.ops.w8_calls)
        ipd["mha"].weight_dtype = "fp8"
        ipd["mha"].seqlen_offset = ipd["hyena"].seqlen_offset = 3
        with pytest.raises(ValueError, match="not a multiple of 256"):
            odd(torch.tensor([[65]] * 9), inference_params_dict=ipd)
    assert odd.ops.w8_calls == calls and m.ops.calls == 0


# ------------------------------------------------------------------------------------------------ 4. resources
def _metadata(src):
    """{kernel name: {vgpr, agpr, sgpr, spill, sgpr_spill, lds, scratch}} from the .amdgpu_metadata of `hipcc -S`."""
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
        def num(key):
            return int(re.search(key + r":\s+(\d+)", blk).group(1))
        res[re.search(r"\.name:\s+(\S+)", blk).group(1)] = {
            "vgpr": num(r"\.vgpr_count"), "sgpr": num(r"\.sgpr_count"), "spill": num(r"\.vgpr_spill_count"),
            "sgpr_spill": num(r"\.sgpr_spill_count"), "lds": num(r"\.group_segment_fixed_size"), "scratch": num(r"\.private_segment_fixed_size")}
    return res


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_the_kernels_need_no_scratch_and_spill_nothing():
    meta = _metadata("skinny_fp8.hip")
    mine = {k: v for k, v in meta.items() if "skinny_w8_kernel" in k}
    # n-split: MT 1-4 x WAVES 2-4; SPLITK and GATE: MT 1-4 at four waves
    assert len(mine) == 12 + 4 + 4 and len(meta) == len(mine) + 1 and any("skinny_reduce_kernel" in k for k in meta), sorted(meta)
    for name, r in meta.items():
        assert r["scratch"] == 0 and r["spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        assert r["lds"] <= 64 * 1024 and r["vgpr"] <= 256, (name, r)       # static LDS; two waves per SIMD or more (the header's table)


# ------------------------------------------------------------------------------------------------ 5. the exact designs at these K
@pytest.mark.parametrize("K", WW.all_reductions())
def test_the_fourbit_design_keeps_every_partial_sum_within_24_bits(K):
    """tests/w8_ref.py:57-62, which does not depend on M: first in integers, then on the data at 64 rows, in two orders of 256-k units."""
    assert K % 256 == 0 and K <= DX.K_MAX
    for u in DX.X_UNITS:
        assert 4 * 15 * K * u < 2 ** 24
        for g in range(W8.W4_G[0], W8.W4_G[1] + 1):
            assert (60 * K * 2.0 ** g + 72) / min(2.0 ** g / u, 0.25) < 2 ** 24, (K, u, g)
    N, M = 32, 64
    w, b, r = W8.make_w4(N, K), DX.make_bias(N), DX.make_residual(M, N)
    rec = Fp8Weight.quantize(w)
    assert torch.equal(rec.dequantize().view(torch.int16), w.view(torch.int16))
    byts = rec.data.view(torch.float8_e4m3fn).float()
    for u in DX.X_UNITS:
        x = DX.make_x(M, K, unit=u)
        S = DX.exact_sum(x, w, b, r)
        fwd, bwd = torch.zeros(M, N), torch.zeros(M, N)
        for k0 in range(0, K, 256):
            fwd = fwd + x[:, k0:k0 + 256].float() @ byts[:, k0:k0 + 256].t()
            k1 = K - 256 - k0
            bwd = bwd + x[:, k1:k1 + 256].float() @ byts[:, k1:k1 + 256].t()
        assert torch.equal(fwd, bwd)
        assert torch.equal((fwd * rec.scale[None, :] + b.float()[None, :] + r.float()).double(), S)


def test_the_slice_rule():
    """include/evo_mi355x.h: slices = min(8, K / 256, ceil(256 / (N / 64))); the GPU module's SPLITK shapes split, its others do not."""
    assert [WW.slices(N, K) for N, K in WW.SPLITK] == [2, 4, 4] and all(WW.slices(N, K) == 1 for N, K in WW.NSPLIT)
    assert WW.slices(4104, 256) == 1 and WW.slices(1536, 512) == 2         # (1536, 512) runs unsplit for want of a workspace only
    for N, K in WW.SPLITK:                                                # every slice holds a unit or more: cuts at floor(units * s / slices)
        units, s = K // 256, WW.slices(N, K)
        cuts = [units * i // s for i in range(s + 1)]
        assert all(b > a for a, b in zip(cuts, cuts[1:])) and cuts[-1] == units
