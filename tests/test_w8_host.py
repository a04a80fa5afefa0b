"""CPU: the opt-in FP8 (e4m3fn) weights for the decode step at 1-8 rows -- the layers that need no GPU.

  * the six C entries: exported, declared, bound, ABI 20, every contract violation refused with -1 before any launch (the pointers
    passed are never dereferenced);
  * THE RULE in torch (evo_amd.sh.cache.fp8_row_rule, which tests/test_gpu_w8.py holds evo_w_quant_fp8 to bit for bit): it is the KV
    cache's rule (tests/test_kv_fp8_host.py quant_rule) on rows of any width; the round trip; row permutations; a = 0; the clamp; row
    maxima on both sides of 448 2^e;
  * exactness of the two designs the GPU module runs on, with the 24-bit bound of the second one proved per K;
  * the model on the fp64 oracle backend (tests/w8_ref.py: the FP8 methods dequantise and call the parent's): weight_dtype="fp8" equals
    the model holding the dequantised weights, in ids and logits (see ON THE TWIN); which tensors got a record; fold_norms_(); two
    generators;
  * every refusal;  * resources of the new kernels from the compiler's metadata.

ON IDEMPOTENCE.  The rule is a fixed point in VALUES: a dequantised row quantises to a record that dequantises to the same values, bit
for bit.  It is a fixed point in (bytes, scale) too unless the row's maximum a 2^-e lies in (224, 232]: that rounds DOWN to the byte 224,
the dequantised row's maximum is 224 2^e, and the smallest exponent with 224 2^e 2^-e' <= 448 is e - 1 -- the second record holds every
byte doubled (exactly representable) under half the scale.  The first test below asserts both statements; the edge has a share of
8 / 224 of the octave.

ON THE TWIN.  An FP8 generation prefills with the bf16 weights W and steps with dq(q(W)); a model that HOLDS dq(q(W)) prefills with
those.  The two can therefore be equal from the first token on only where W = dq(q(W)) already.  So the equality is asserted in the two
forms in which it is true, both by torch.equal in ids and logits: (a) on the twin -- the model holding the dequantised weights --
weight_dtype="fp8" equals weight_dtype="bf16" through Generator, generate() and a 4-slot pool, prefill included; (b) on the original
model, from one bf16 prefill whose cache is copied, the FP8 steps equal the twin's bf16 steps."""
import ctypes
import os
import re

import pytest
import torch

import dense_exact as DX
import w8_ref as W8
from evo_amd import _build
from evo_amd import ops as evo_ops
from evo_amd.backend import Backend
from evo_amd.generation import Generator, generate
from evo_amd.pool import DecodePool, sample_many
from evo_amd.sh.cache import Fp8Weight, InferenceParams, check_weight_dtype, fp8_row_rule
from test_gpu_pool import PROMPTS
from test_kernel_resources import HIPCC, _metadata
from test_kv_fp8_host import quant_rule
from test_ragged_prefill_host import SMALL, TOK

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("evo_w_quant_fp8", "evo_linear_small_m_w8", "evo_norm_linear_small_m_w8", "evo_hyena_decode_fused_small_m_w8",
           "evo_mlp_gate_small_m_w8", "evo_norm_mlp_gate_small_m_w8")


# ------------------------------------------------------------------------------------------------ wiring and refusals
def test_entries_are_wired():
    header = open(os.path.join(ROOT, "include", "evo_mi355x.h")).read()
    for name in ENTRIES:
        assert name in _build.EXPORTS and name in evo_ops._SIGNATURES and re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert int(re.search(r"#define EVO_ABI_VERSION (\d+)", header).group(1)) == evo_ops.ABI_VERSION == 20
    assert evo_ops.load_library().evo_abi_version() == 20
    for meth in Backend.OPTIONAL["w_fp8"]:
        assert hasattr(evo_ops.HipOps, meth), meth
    assert any(p.name == "gemv_fp8.hip" for p in _build.sources())
    assert InferenceParams(max_seqlen=8, max_batch_size=1).weight_dtype == "bf16"
    for script, flag in (("sample_many.py", "--weight-dtype"), ("generate.py", "--weight-dtype")):
        text = open(os.path.join(ROOT, "scripts", script)).read()
        assert flag in text and "weight_dtype" in text, script


ONE = ctypes.c_void_p(16)                                             # non-null, 16-byte aligned, never dereferenced
F = ctypes.c_float
BAD_SHAPES = [dict(M=0), dict(M=9), dict(M=-1), dict(K=0), dict(K=8), dict(K=4104), dict(K=-16)]


def _caller(name, names, ok):
    f = getattr(evo_ops.load_library(), name)
    assert list(ok) == names and len(evo_ops._SIGNATURES[name][0]) == len(names)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return f(*[a[n] for n in names])
    return call


def _refuses(call, required, optional=(), sizes=(), scale_name="w_scale"):
    for n in required:
        assert call(**{n: None}) == -1, n
        bad = ctypes.c_void_p(18) if n == scale_name else ctypes.c_void_p(8)
        assert call(**{n: bad}) == -1, n
    for n in optional:
        assert call(**{n: ctypes.c_void_p(8)}) == -1, n
    for kw in list(sizes) + BAD_SHAPES:
        assert call(**kw) == -1, kw


def test_compute_entries_refuse_before_any_launch():
    ok = dict(x=ONE, w_data=ONE, w_scale=ONE, bias=ONE, residual=ONE, y=ONE, M=2, N=64, K=32, ws=None, ws_bytes=0, stream=None)
    _refuses(_caller("evo_linear_small_m_w8", list(ok), ok), ("x", "w_data", "w_scale", "y"), ("bias", "residual"), [dict(N=0), dict(N=-4)])
    ok = dict(x=ONE, scale=ONE, w_data=ONE, w_scale=ONE, bias=ONE, y=ONE, M=2, N=64, K=32, eps=F(1e-6), stream=None)
    _refuses(_caller("evo_norm_linear_small_m_w8", list(ok), ok), ("x", "scale", "w_data", "w_scale", "y"), ("bias",),
             [dict(N=0), dict(M=5), dict(M=8, K=4080)])              # 5-8 rows: K = 4096 only
    ok = dict(x=ONE, norm_scale=ONE, proj_data=ONE, proj_scale=ONE, proj_b=ONE, fir_state=ONE, iir_state=ONE, fir_w=ONE, fir_b=ONE, poles=ONE,
              residues=ONE, dskip=ONE, y=ONE, M=2, D=256, n_heads=2, eps=F(1e-6), stream=None)
    call = _caller("evo_hyena_decode_fused_small_m_w8", list(ok), ok)
    _refuses(lambda **kw: call(**{("D" if k == "K" else k): v for k, v in kw.items()}),
             [n for n in ok if ok[n] is ONE], (), [dict(n_heads=3), dict(D=0), dict(M=5)], scale_name="proj_scale")
    ok = dict(x=ONE, w12_data=ONE, w12_scale=ONE, a=ONE, M=2, I=64, K=32, grouped=0, stream=None)
    _refuses(_caller("evo_mlp_gate_small_m_w8", list(ok), ok), ("x", "w12_data", "w12_scale", "a"), (),
             [dict(I=0), dict(I=63), dict(I=40, grouped=1)], scale_name="w12_scale")
    ok = dict(x=ONE, scale=ONE, w12_data=ONE, w12_scale=ONE, a=ONE, M=2, I=64, K=32, eps=F(1e-6), grouped=0, stream=None)
    _refuses(_caller("evo_norm_mlp_gate_small_m_w8", list(ok), ok), ("x", "scale", "w12_data", "w12_scale", "a"), (),
             [dict(I=0), dict(I=63), dict(M=5), dict(I=40, grouped=1)], scale_name="w12_scale")
    ok = dict(w=ONE, w_data=ONE, w_scale=ONE, N=4, K=32, stream=None)
    call = _caller("evo_w_quant_fp8", list(ok), ok)
    for n in ("w", "w_data", "w_scale"):
        assert call(**{n: None}) == -1 and call(**{n: ctypes.c_void_p(18 if n == "w_scale" else 8)}) == -1, n
    for kw in (dict(N=0), dict(N=-1), dict(K=0), dict(K=8), dict(K=24)):
        assert call(**kw) == -1, kw


# ------------------------------------------------------------------------------------------------ the rule
def _rows(seed=0, N=4000, K=48):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-30, 30, (N, 1), generator=g).float())).bfloat16()


def test_the_rule_is_the_kv_rule_and_a_fixed_point_in_values():
    w = torch.cat([_rows(), W8.quant_rows(37, 48)])
    data, scale = fp8_row_rule(w)
    kd, ks = quant_rule(w)                                            # tests/test_kv_fp8_host.py: the rule ABI 19's kernels are held to
    assert torch.equal(data, kd) and torch.equal(scale, ks)
    rec = Fp8Weight(data, scale)
    deq = rec.dequantize()
    assert deq.dtype == torch.bfloat16 and torch.equal(deq.float(), rec.dequantize(torch.float32))      # byte * scale is a bf16 number
    again = Fp8Weight.quantize(deq)
    assert torch.equal(again.dequantize().view(torch.int16), deq.view(torch.int16))                      # the fixed point, in values
    # ... and in (bytes, scale) except where the row's scaled maximum rounds down to 224 (module docstring)
    top = (w.float().abs().amax(1) / scale)
    edge = (top > 224) & (top <= 232)
    same = (again.data == data).all(1) & (again.scale == scale)
    assert bool(same[~edge].all()) and 0 < int(edge.sum()) < 0.08 * len(w)
    assert bool((again.scale[edge] * 2 == scale[edge]).all()) and not bool(same[edge].any())


def test_the_rule_commutes_with_row_permutations():
    w = _rows(1, 500, 32)
    perm = torch.randperm(500, generator=torch.Generator().manual_seed(2))
    d, s = fp8_row_rule(w)
    dp, sp = fp8_row_rule(w[perm])
    assert torch.equal(dp, d[perm]) and torch.equal(sp, s[perm])
    # the grouped l1 | l2 order is such a permutation
    w12 = _rows(3, 128, 32)
    g = Backend.pack_gate_weights(w12)
    dg, sg = fp8_row_rule(g)
    d, s = fp8_row_rule(w12)
    assert torch.equal(dg, Backend.pack_gate_weights(d)) and torch.equal(sg, Backend.pack_gate_weights(s[:, None])[:, 0])


def test_zero_rows_the_clamp_and_both_sides_of_448():
    K = 16
    def row(top):
        r = torch.full((K,), top / 4)
        r[-1] = top                                                   # (the maximum is the last element)
        return r
    tops = [0.0, 448.0, 450.0, 446.0, 1.75, 1.7578125, 1.7421875, 2.0 ** -130, 2.0 ** -126 * 1.75, 2.0 ** 127, 3.0e38]
    w = torch.stack([row(t) for t in tops]).bfloat16()
    data, scale = fp8_row_rule(w)
    e = torch.log2(scale).tolist()
    #        0   448  450->e=1  446  1.75  >1.75  <1.75   clamp  clamp   2^127  ~2^128
    assert e == [0.0, 0.0, 1.0, 0.0, -8.0, -7.0, -8.0, -126.0, -126.0, 119.0, 120.0], e
    assert not bool(data[0].any())                                    # a = 0: zero bytes under scale 1
    v = data.view(torch.float8_e4m3fn).float()
    assert float(v.abs().max()) <= 448 and bool(torch.isfinite(v).all())
    assert v[1, -1] == 448 and v[2, -1] == 224 and v[4, -1] == 448 and v[5, -1] == 224 and v[7, -1] == 2.0 ** -4
    # the smallest integer: one less would overflow 448 (where the clamp does not bind)
    a = w.float().abs().amax(1).double()
    free = (scale > 2.0 ** -126) & (a > 0)
    assert bool((a[free] / scale[free].double() <= 448).all()) and bool((a[free] / scale[free].double() * 2 > 448).all())


# ------------------------------------------------------------------------------------------------ the two designs
@pytest.mark.parametrize("design", list(W8.DESIGNS))
def test_the_designs_dequantise_to_themselves(design):
    make_w, make_gate = W8.DESIGNS[design]
    for w in (make_w(300, 11008), make_w(37, 16), make_gate(64, 4096), make_gate(1408, 272)):
        rec = Fp8Weight.quantize(w)
        assert torch.equal(rec.dequantize().view(torch.int16), w.view(torch.int16))
        assert bool((torch.log2(rec.scale) == torch.log2(rec.scale).round()).all())
    if design == "fourbit":                                           # it uses the format: all four significant bits, several row scales
        w = make_w(300, 4096)
        rec = Fp8Weight.quantize(w)
        m = rec.data.view(torch.float8_e4m3fn).float().abs()
        frac = m / torch.exp2(torch.floor(torch.log2(m.clamp_min(2.0 ** -20))))
        assert set(frac[m > 0].unique().tolist()) == {1 + i / 8 for i in range(8)}
        assert len(rec.scale.unique()) >= W8.W4_G[1] - W8.W4_G[0]


@pytest.mark.parametrize("K", W8.all_reductions())
def test_the_fourbit_design_keeps_every_partial_sum_within_24_bits(K):
    """The bound of tests/w8_ref.py, first in integers, then on the data: fp32 == fp64 in two summation orders."""
    assert K % 16 == 0 and K <= DX.K_MAX
    for u in DX.X_UNITS:
        assert 4 * 15 * K * u < 2 ** 24                                # the byte-domain sum, in units of 1 / u
        for g in range(W8.W4_G[0], W8.W4_G[1] + 1):                    # + bias + residual after the row's 2^g, in units of min(2^g / u, 1/4)
            unit = min(2.0 ** g / u, 0.25)
            assert (60 * K * 2.0 ** g + 72) / unit < 2 ** 24, (K, u, g)
    if K in (256, 1024, 4096):                                         # the norm-folding forms' x: integers in [-6, 6] (make_norm_rows), + bias
        for g in range(W8.W4_G[0], W8.W4_G[1] + 1):
            assert 90 * K < 2 ** 24 and (90 * K * 2.0 ** g + 8) / min(2.0 ** g, 0.25) < 2 ** 24
    N, M = 64, 8
    w, b, r = W8.make_w4(N, K), DX.make_bias(N), DX.make_residual(M, N)
    rec = Fp8Weight.quantize(w)
    byts = rec.data.view(torch.float8_e4m3fn).float()
    for u in DX.X_UNITS:
        x = DX.make_x(M, K, unit=u)
        S = DX.exact_sum(x, w, b, r)                                   # (asserts that the sum is an fp32 number)
        fwd = torch.zeros(M, N)
        bwd = torch.zeros(M, N)
        for k0 in range(0, K, 16):                                     # the kernels' grain: 16 weights at a time, forwards and backwards
            fwd = fwd + x[:, k0:k0 + 16].float() @ byts[:, k0:k0 + 16].t()
            k1 = K - 16 - k0
            bwd = bwd + x[:, k1:k1 + 16].float() @ byts[:, k1:k1 + 16].t()
        assert torch.equal(fwd, bwd)
        for acc in (fwd, bwd):
            out = acc * rec.scale[None, :] + b.float()[None, :] + r.float()
            assert torch.equal(out.double(), S)


# ------------------------------------------------------------------------------------------------ the model on the fp64 oracle backend
def _model(ops, cfg=SMALL, seed=3):
    from oracle.stripedhyena_ref import RefConfig, make_synthetic_state_dict
    from evo_amd.sh.model import StripedHyena
    sd = make_synthetic_state_dict(RefConfig.from_dict(cfg), seed=seed)
    m = StripedHyena(dict(cfg), ops=ops)
    m.load_state_dict({k: (v.double() if v.dtype == torch.bfloat16 else v) for k, v in sd.items()})
    return m


STREAMED = ("projections.weight", "Wqkv.weight", "out_filter_dense.weight", "out_proj.weight", "l1.weight", "l2.weight", "l3.weight")


def _dequantised_twin(m):
    """The same model with every streamed weight replaced by its dequantised value (and nothing else changed)."""
    twin = _model(W8.W8OracleOps(torch.float64))
    sd = {}
    for k, v in m.state_dict().items():
        sd[k] = Fp8Weight.quantize(v).dequantize(torch.float64) if k.endswith(STREAMED) else v.clone()
    twin.load_state_dict(sd)
    return twin


@pytest.fixture(scope="module")
def small():
    return _model(W8.W8OracleOps(torch.float64))


@pytest.fixture(scope="module")
def twin(small):
    return _dequantised_twin(small)


def _gen(model, weight_dtype, prompts, n=6, **kw):
    g = Generator(model, TOK, top_k=1, top_p=1.0, temperature=0.0, weight_dtype=weight_dtype, **kw)
    ids = torch.tensor([list(p.encode()) for p in prompts])
    return g.generate("cpu", input_ids=ids, num_tokens=n, cached_generation=True, print_generation=False, stop_at_eos=False)


def _steps(model, ipd, first, fmt, n):
    """n greedy single-token steps of `model` on the cache `ipd` in format `fmt`, from the tokens `first` [B] -> (ids [B, n], logits)."""
    ipd["mha"].weight_dtype = fmt
    off, tok, ids, rows = int(ipd["_len"]), first, [], []
    for _ in range(n):
        ipd["mha"].seqlen_offset = ipd["hyena"].seqlen_offset = off
        with torch.inference_mode():
            logits, _ = model(tok[:, None], inference_params_dict={"mha": ipd["mha"], "hyena": ipd["hyena"]})
        off += 1
        tok = logits[:, -1].argmax(-1)
        ids.append(tok)
        rows.append(logits[:, -1].float())
    return torch.stack(ids, 1), torch.stack(rows, 1)


def _steps_equal_the_twins(model, twin_model, prompts, n=5):
    """(b) of the module docstring: ONE bf16 prefill on `model`, its cache copied; FP8 steps on `model` == bf16 steps on the twin."""
    import copy
    ids = torch.tensor([list(p.encode()) for p in prompts])
    ipd = model.initialize_inference_params()
    ipd["mha"].max_batch_size = ipd["hyena"].max_batch_size = len(prompts)
    with torch.inference_mode():
        logits, ipd = model(ids, inference_params_dict=ipd)
    first = logits[:, -1].argmax(-1)
    a, b = dict(copy.deepcopy(ipd), _len=ids.shape[1]), dict(copy.deepcopy(ipd), _len=ids.shape[1])
    ids8, logits8 = _steps(model, a, first, "fp8", n)
    idsd, logitsd = _steps(twin_model, b, first, "bf16", n)
    assert torch.equal(ids8, idsd) and torch.equal(logits8, logitsd)
    ids16, logits16 = _steps(model, dict(copy.deepcopy(ipd), _len=ids.shape[1]), first, "bf16", n)
    assert not torch.equal(logits8, logits16)                         # (the format is not a no-op on these weights)
    return logits8


def test_generate_equals_the_model_on_dequantised_weights(small, twin):
    prompts = ["ACGTTGCA", "GGATTACA", "TTTTACGA"]
    _steps_equal_the_twins(small, twin, prompts)
    # (a) on the twin, through the public interface
    twin.ops.w8_calls = dict.fromkeys(twin.ops.w8_calls, 0)
    ids8, logits8, ipd = _gen(twin, "fp8", prompts)
    c = dict(twin.ops.w8_calls)
    idsd, logitsd, _ = _gen(twin, "bf16", prompts)
    assert torch.equal(ids8, idsd) and torch.equal(logits8, logitsd)
    assert ipd["mha"].weight_dtype == "fp8" and twin.ops.w8_calls == c  # (the bf16 run made no FP8 call)
    steps, L, A = 5, twin.num_layers, len(twin.attn_layer_idxs)
    assert c["hyena"] == steps * (L - A) and c["norm_linear"] == steps * A and c["gate"] == steps * L and c["linear"] == 2 * steps * L
    assert c["quant"] == 4 * L
    # the prefill of an FP8 generation is the bf16 prefill: on the ORIGINAL model the first logits are the bf16 run's, the later ones not
    o8, ol8, _ = _gen(small, "fp8", prompts)
    o16, ol16, _ = _gen(small, "bf16", prompts)
    assert torch.equal(ol8[:, 0], ol16[:, 0]) and torch.equal(o8[:, 0], o16[:, 0]) and not torch.equal(ol8[:, 1:], ol16[:, 1:])
    # the public function
    s8, _ = generate(prompts, twin, TOK, n_tokens=4, cached_generation=True, device="cpu", verbose=0, weight_dtype="fp8")
    sd, _ = generate(prompts, twin, TOK, n_tokens=4, cached_generation=True, device="cpu", verbose=0)
    assert s8 == sd


def test_which_tensors_got_a_record(small):
    small.prepare_fp8_weights()
    D, inner = small.hidden_size, small.inner_size
    assert len(small._w8) == small.num_layers
    for i, layer in enumerate(small._w8):
        assert sorted(layer) == ["in", "out", "w12", "w3"]
        assert tuple(layer["in"].shape) == (3 * D, D) and tuple(layer["out"].shape) == (D, D)
        assert tuple(layer["w12"].shape) == (2 * inner, D) and tuple(layer["w3"].shape) == (D, inner)
        for rec in layer.values():
            assert rec.data.dtype == torch.uint8 and rec.scale.dtype == torch.float32 and rec.scale.shape == (rec.data.shape[0],)
            assert rec.nbytes() == rec.data.numel() + 4 * rec.data.shape[0]
    per_block = 3 * D * D + D * D + 2 * inner * D + D * inner
    rows = 3 * D + D + 2 * inner + D
    emb = small.unembed.weight.numel() * small.unembed.weight.element_size()
    assert small.decode_weight_bytes("fp8") == small.num_layers * (per_block + 4 * rows) + emb
    assert small.decode_weight_bytes("bf16") == small.num_layers * per_block * small.blocks[0].mlp._w3.element_size() + emb
    # the embedding / unembedding, biases, norm scales, FIR taps, poles and residues have none: nothing but the four per block
    held = {id(r.data) for layer in small._w8 for r in layer.values()}
    assert len(held) == 4 * small.num_layers


@pytest.mark.parametrize("share_prompt_kv", [False, True])
def test_pool_of_four_slots_equals_the_dequantised_twin(small, twin, share_prompt_kv):
    kw = dict(n_slots=4, top_k=1, top_p=1.0, temperature=0.0, device="cpu", share_prompt_kv=share_prompt_kv)
    twin.ops.w8_calls = dict.fromkeys(twin.ops.w8_calls, 0)
    p8 = DecodePool(twin, TOK, weight_dtype="fp8", **kw)
    s8, sc8, o8 = p8.generate(PROMPTS, n_tokens=5, n_sample_per_prompt=1)
    c = dict(twin.ops.w8_calls)
    pd = DecodePool(twin, TOK, **kw)
    sd, scd, od = pd.generate(PROMPTS, n_tokens=5, n_sample_per_prompt=1)
    assert s8 == sd and o8 == od and sc8 == scd
    for a, b in zip(p8.last_logits, pd.last_logits):
        assert torch.equal(a, b)
    L = twin.num_layers
    assert twin.ops.w8_calls == c and c["gate"] == p8.stats["steps"] * L > 0 and c["linear"] == 2 * p8.stats["steps"] * L
    assert p8.stats["weight_dtype"] == "fp8" and pd.stats["weight_dtype"] == "bf16"
    assert p8.stats["decode_weight_bytes"] == twin.decode_weight_bytes("fp8") < pd.stats["decode_weight_bytes"]
    assert p8.ipd["mha"].weight_dtype == "fp8" and pd.ipd["mha"].weight_dtype == "bf16"
    # on the original model the pool runs the FP8 steps too (its prefills read the bf16 weights: other tokens than the twin's may follow)
    small.ops.w8_calls = dict.fromkeys(small.ops.w8_calls, 0)
    DecodePool(small, TOK, weight_dtype="fp8", **kw).generate(PROMPTS[:2], n_tokens=3, n_sample_per_prompt=1)
    assert small.ops.w8_calls["gate"] > 0
    # sample_many passes the option on
    _, seqs, _ = sample_many(PROMPTS[:2], twin, TOK, n_tokens=3, temp=0.0, top_k=1, n_slots=2, device="cpu", weight_dtype="fp8",
                             share_prompt_kv=share_prompt_kv)
    assert seqs == [x[:3] for x in s8[:2]]


def test_beam_search_runs_fp8_steps_and_leaves_the_flag_as_the_pool_set_it():
    """A share_prompt_kv pool's caches carry the pool's weight format themselves: the search patches nothing for its run."""
    from beam_ref import BeamOracleOps

    class BeamW8Ops(W8.W8OracleOps, BeamOracleOps):
        pass
    m = _model(BeamW8Ops(torch.float64))
    pool = DecodePool(m, TOK, n_slots=4, device="cpu", share_prompt_kv=True, weight_dtype="fp8")
    res = pool.beam_search(PROMPTS[:2], 3, beam_width=2)
    L, steps = m.num_layers, pool.stats["beam_steps"]
    assert len(res) == 2 and steps > 0
    assert m.ops.w8_calls["gate"] == steps * L and m.ops.w8_calls["linear"] == 2 * steps * L
    assert pool.ipd["mha"].weight_dtype == "fp8"


def test_a_set_built_before_fold_norms_is_rebuilt_after_it():
    m = _model(W8.W8OracleOps(torch.float64), seed=5)
    for blk in m.blocks:                                              # (non-trivial norm scales: the fold changes the weights)
        blk.pre_norm.scale.data = blk.pre_norm.scale.data * 1.25
        blk.post_norm.scale.data = blk.post_norm.scale.data * 0.75
    m.prepare_fp8_weights()
    before = m._w8
    m.fold_norms_()
    assert m._w8 is None
    folded_twin = _model(W8.W8OracleOps(torch.float64), seed=5)
    sd = {k: (Fp8Weight.quantize(v).dequantize(torch.float64) if k.endswith(STREAMED) else v.clone()) for k, v in m.state_dict().items()}
    folded_twin.load_state_dict(sd)
    _steps_equal_the_twins(m, folded_twin, ["ACGTTGCA", "GGATTACA"])
    assert m._w8 is not None and m._w8 is not before
    assert not torch.equal(m._w8[0]["in"].data, before[0]["in"].data)
    # .to(...) and a new state dict drop a set as well
    m2 = _model(W8.W8OracleOps(torch.float64)).prepare_fp8_weights()
    m2.to("cpu")
    assert m2._w8 is None
    m2.prepare_fp8_weights().load_state_dict(m2.state_dict())
    assert m2._w8 is None


def test_two_generators_with_different_formats_interleave(small, twin):
    """One model, two generations alive at once, stepped alternately by hand: each equals its own uninterrupted run."""
    prompt = torch.tensor([list(b"ACGTTGCAAC")])
    want8, wantl8, _ = _gen(small, "fp8", ["ACGTTGCAAC"], n=5)
    want16, wantl16, _ = _gen(small, "bf16", ["ACGTTGCAAC"], n=5)
    runs = {}
    for fmt in ("fp8", "bf16"):
        ipd = small.initialize_inference_params()
        ipd["mha"].weight_dtype = fmt
        with torch.inference_mode():
            logits, ipd = small(prompt, inference_params_dict=ipd)
        runs[fmt] = dict(ipd=ipd, off=prompt.shape[1], toks=[int(logits[0, -1].argmax())], rows=[logits[0, -1].float()])
    for _ in range(4):
        for fmt in ("fp8", "bf16"):
            r = runs[fmt]
            r["ipd"]["mha"].seqlen_offset = r["ipd"]["hyena"].seqlen_offset = r["off"]
            with torch.inference_mode():
                logits, _ = small(torch.tensor([[r["toks"][-1]]]), inference_params_dict=r["ipd"])
            r["off"] += 1
            r["toks"].append(int(logits[0, -1].argmax()))
            r["rows"].append(logits[0, -1].float())
    assert runs["fp8"]["toks"] == want8[0].tolist() and torch.equal(torch.stack(runs["fp8"]["rows"]), wantl8[0])
    assert runs["bf16"]["toks"] == want16[0].tolist() and torch.equal(torch.stack(runs["bf16"]["rows"]), wantl16[0])
    assert not torch.equal(wantl8[0, 1:], wantl16[0, 1:])


# ------------------------------------------------------------------------------------------------ refusals
class _CountingOps(W8.W8OracleOps):
    """Counts every kernel-level call: a refusal must come before the first one."""

    def __init__(self):
        super().__init__(torch.float64)
        self.calls = 0

    def embed(self, *a, **kw):
        self.calls += 1
        return super().embed(*a, **kw)

    def w_quant_fp8(self, w):
        self.calls += 1
        return super().w_quant_fp8(w)


def test_every_refusal_comes_before_any_device_work():
    from test_ragged_prefill_host import RaggedOracleOps
    m = _model(_CountingOps())
    # an unknown value
    for make in (lambda: Generator(m, TOK, weight_dtype="fp4"), lambda: DecodePool(m, TOK, n_slots=2, device="cpu", weight_dtype="int8"),
                 lambda: generate(["ACGT"], m, TOK, n_tokens=2, device="cpu", verbose=0, weight_dtype="e5m2"),
                 lambda: sample_many(["ACGT"], m, TOK, n_tokens=2, device="cpu", weight_dtype="FP8"), lambda: check_weight_dtype(None)):
        with pytest.raises(ValueError, match="weight_dtype"):
            make()
    # more than 8 rows
    with pytest.raises(ValueError, match="at most 8"):
        DecodePool(m, TOK, n_slots=9, device="cpu", weight_dtype="fp8")
    with pytest.raises(ValueError, match="at most 8"):
        generate(["ACGTACGT"] * 9, m, TOK, n_tokens=2, cached_generation=True, device="cpu", verbose=0, weight_dtype="fp8")
    with pytest.raises(ValueError, match="at most 8"):
        Generator(m, TOK, weight_dtype="fp8").generate("cpu", input_ids=torch.zeros(9, 4, dtype=torch.long), num_tokens=2)
    DecodePool(m, TOK, n_slots=8, device="cpu", weight_dtype="fp8")
    # a streamed layer whose K is not a multiple of 16: named
    odd = _model(_CountingOps(), cfg=dict(SMALL, inner_mlp_size=680))
    for make in (lambda: Generator(odd, TOK, weight_dtype="fp8"), lambda: DecodePool(odd, TOK, n_slots=2, device="cpu", weight_dtype="fp8"),
                 odd.prepare_fp8_weights):
        with pytest.raises(ValueError, match=r"blocks\.0\.mlp\.l3 has K = 680"):
            make()
    # a backend without the group
    plain = _model(RaggedOracleOps(torch.float64))
    for make in (lambda: Generator(plain, TOK, weight_dtype="fp8"), lambda: DecodePool(plain, TOK, n_slots=2, device="cpu", weight_dtype="fp8"),
                 plain.prepare_fp8_weights):
        with pytest.raises(RuntimeError, match="w_fp8"):
            make()
    ipd = plain.initialize_inference_params()
    with torch.inference_mode():
        _, ipd = plain(torch.tensor([[65, 67, 71]]), inference_params_dict=ipd)
        ipd["mha"].weight_dtype = "fp8"
        ipd["mha"].seqlen_offset = ipd["hyena"].seqlen_offset = 3
        with pytest.raises(RuntimeError, match="w_fp8"):
            plain(torch.tensor([[65]]), inference_params_dict=ipd)
        ipd["mha"].weight_dtype = "fp4"
        with pytest.raises(ValueError, match="weight_dtype"):
            plain(torch.tensor([[65]]), inference_params_dict=ipd)
    assert m.ops.calls == 0 and odd.ops.calls == 0


# ------------------------------------------------------------------------------------------------ resources
def _waves(vgpr):
    """Waves per SIMD the register count allows on gfx950 (512 VGPRs per lane, allocated in blocks of 8, at most 8 waves)."""
    return min(8, 512 // ((vgpr + 7) // 8 * 8))


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_fp8_kernels_need_no_scratch_and_keep_their_siblings_occupancy():
    fp8, bf16 = _metadata("gemv_fp8.hip"), _metadata("gemv.hip")
    assert any("w_quant_fp8_kernel" in k for k in fp8)
    pairs = 0
    for name, r in fp8.items():
        assert r["scratch"] == 0 and r["spill"] == 0 and r["sgpr_spill"] == 0, (name, r)
        m = re.match(r"_Z\d+w8_(gemv\w*?_kernel)(I.*?E)vPK", name)
        if m is None:
            assert "w_quant_fp8_kernel" in name, name
            continue
        sib = [v for k, v in bf16.items() if re.match(r"_Z\d+" + m.group(1) + re.escape(m.group(2)) + "vPK", k)]
        if not sib:                                                   # the gate without the norm at 5-8 rows: bf16 hands those to its MFMA form
            assert "gemv_gate_kernel" in name and "Lb0ELb0E" in name and int(re.search(r"ILi(\d)E", name).group(1)) >= 5, name
            continue
        pairs += 1
        assert r["lds"] <= sib[0]["lds"], (name, r, sib[0])             # (static LDS; the staged rows are dynamic, M K 2 bytes in both)
        assert _waves(r["vgpr"]) >= _waves(sib[0]["vgpr"]), (name, r["vgpr"], sib[0]["vgpr"])
    assert pairs == 16 + 12 + 12 + 12 + 4                             # gemv 8 x {SPLIT, not}; norm, Hyena, gate + norm: 8 + 4; gate: 4 of 8
