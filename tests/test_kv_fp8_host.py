"""CPU: the opt-in FP8 (e4m3fn) KV cache for decode -- the layers that need no GPU.

  * the three C entries: exported, declared, bound, ABI >= 19, every contract violation refused with -1 before any launch (the pointers
    passed are never dereferenced);
  * THE RULE in torch (`quant_rule` below, which tests/test_gpu_kv_fp8.py holds the kernels to bit for bit): its exponent against brute
    force over range(-126, 121) on adversarial row maxima, exactness of the dequantised values and idempotence of the round trip;
  * the scheduler and the model plumbing on the fp64 oracle backend with the three methods written from the rule: DecodePool(kv_dtype=
    "fp8"), greedy, against a one-job-at-a-time loop (prefill, then single steps on an FP8 cache); `stats["kv_bytes"]`; Generator; the
    refused combinations;
  * resources: the new kernels without scratch or spills."""
import ctypes
import os
import re
from fractions import Fraction

import pytest
import torch

from evo_amd import _build
from evo_amd import ops as evo_ops
from evo_amd.backend import Backend
from evo_amd.generation import Generator
from evo_amd.pool import DecodePool, sample_many
from evo_amd.sh.cache import Fp8KV, InferenceParams
from test_gpu_pool import PROMPTS
from test_kernel_resources import HIPCC, _metadata
from test_ragged_prefill_host import SMALL, TOK, RaggedOracleOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("evo_kv_quant_fp8", "evo_rope_append_decode_fp8", "evo_attn_decode_fp8")
E_MIN, E_MAX, FP8_MAX = -126, 120, 448


# ------------------------------------------------------------------------------------------------ the rule, in torch
def pow2_f32(e: torch.Tensor) -> torch.Tensor:
    """2^e as f32 from its bit pattern, e an integer tensor in [-126, 127]: exact by construction."""
    return ((e.to(torch.int32) + 127) << 23).view(torch.float32)


def rule_exponent(a: torch.Tensor) -> torch.Tensor:
    """e of the rule for row maxima a >= 0 (any float dtype): a = m 2^x with m in [0.5, 1) (frexp); e = x - 9 if m <= 0.875 else x - 8,
    clamped to [-126, 120]; a = 0 gives 0."""
    m, x = torch.frexp(a.double())
    e = torch.where(m <= 0.875, x - 9, x - 8).clamp(E_MIN, E_MAX)
    return torch.where(a == 0, torch.zeros_like(e), e).to(torch.int32)


def quant_rule(x: torch.Tensor):
    """Rows x [..., 128] -> (bytes [..., 128] uint8 (e4m3fn bit patterns), scale [...] f32 = 2^e).  For bf16 rows this is the reference the
    kernels must equal bit for bit: the product with 2^-e is exact in fp32, the conversion is torch's round-to-nearest-even."""
    e = rule_exponent(x.abs().amax(-1))
    scaled = x.float() * pow2_f32(-e).unsqueeze(-1) if x.dtype != torch.float64 else (x * pow2_f32(-e).double().unsqueeze(-1)).float()
    return scaled.to(torch.float8_e4m3fn).view(torch.uint8), pow2_f32(e)


def dequant(byts: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    return byts.view(torch.float8_e4m3fn).float() * scale.unsqueeze(-1)


def bf16_ulp_neighbours(v: float):
    """(the bf16 below v, v, the bf16 above v) for a positive bf16-representable v."""
    bits = int(torch.tensor(v, dtype=torch.bfloat16).view(torch.int16))
    return [float(torch.tensor(b, dtype=torch.int16).view(torch.bfloat16)) for b in (bits - 1, bits, bits + 1)]


def adversarial_maxima():
    """Row maxima at which an off-by-one exponent shows: 448 2^k exactly and one bf16 ulp to either side, the smallest bf16 subnormal, 3e38."""
    out = []
    for k in list(range(-134, -118)) + list(range(-12, 13)) + list(range(108, 120)):
        v = 448.0 * 2.0 ** k
        if 2.0 ** -133 < v < 3.3e38:
            out += bf16_ulp_neighbours(v)
    out += [2.0 ** -133, float(torch.tensor(3e38, dtype=torch.bfloat16)), 1.0, 0.875, 0.87890625, 1.75, 1.7578125]
    return out


def test_the_exponent_of_the_rule_against_brute_force():
    maxima = adversarial_maxima()
    a = torch.tensor(maxima, dtype=torch.bfloat16)
    assert a.float().tolist() == maxima                              # all of them are bf16 values
    got = rule_exponent(a).tolist()
    for v, e in zip(maxima, got):
        brute = min(k for k in range(E_MIN, E_MAX + 1) if Fraction(v) / Fraction(2) ** k <= FP8_MAX)
        assert e == brute, (v, e, brute)
    assert rule_exponent(torch.zeros(1, dtype=torch.bfloat16)).tolist() == [0]
    assert min(got) == E_MIN and max(got) == E_MAX                   # both clamps are exercised
    # 448 2^k itself sits at the top of its exponent, one ulp above needs the next
    lo, mid, hi = (rule_exponent(torch.tensor([v], dtype=torch.bfloat16)).item() for v in bf16_ulp_neighbours(448.0))
    assert (lo, mid, hi) == (0, 0, 1)


def adversarial_rows(n_random=64, seed=0):
    """[n, 128] bf16: N(0, 1) rows, rows scaled by 1e-6 and by 1e4, an all-zero row, rows whose maximum is each adversarial maximum (at a
    random place and sign, the rest N(0, 1) scaled below it), rows with -0.0 elements."""
    g = torch.Generator().manual_seed(seed)
    base = torch.randn(n_random, 128, generator=g)
    rows = [base, base * 1e-6, base * 1e4, torch.zeros(1, 128)]
    for v in adversarial_maxima():
        r = torch.randn(128, generator=g)
        r = r / r.abs().max() * min(v, 1e38) * 0.99
        r = r.to(torch.bfloat16).float().clamp(-v, v)
        j = int(torch.randint(0, 128, (1,), generator=g))
        r[j] = v if j % 2 else -v
        rows.append(r[None])
    z = torch.randn(2, 128, generator=g)
    z[:, ::3] = -0.0
    rows += [z, torch.full((1, 128), -0.0)]
    return torch.cat(rows).to(torch.bfloat16)


def test_the_rule_is_exact_and_idempotent():
    x = adversarial_rows()
    assert bool(torch.isfinite(x.float()).all())
    byts, scale = quant_rule(x)
    e = rule_exponent(x.abs().amax(-1))
    # the scaled row is exact in fp32 and never beyond 448: the conversion neither saturates nor meets NaN (0x7f / 0xff)
    exact = x.double() * (2.0 ** (-e.double())).unsqueeze(-1)
    assert torch.equal((x.float() * pow2_f32(-e).unsqueeze(-1)).double(), exact) and float(exact.abs().max()) <= FP8_MAX
    assert not bool(((byts & 0x7f) == 0x7f).any())
    # e is the SMALLEST such exponent: a row's scaled maximum lies in (224, 448], bytes 0x76 (224) ... 0x7e (448), unless e sits at its clamp
    nz = (x.abs().amax(-1) > 0) & (e > E_MIN)
    assert bool(nz.any()) and bool(((byts & 0x7f).amax(-1)[nz] >= 0x76).all())
    # byte * scale is exact in fp32 (an fp8 value has 4 significant bits, the scale is a power of two)
    deq = dequant(byts, scale)
    assert torch.equal(deq.double(), byts.view(torch.float8_e4m3fn).double() * scale.double().unsqueeze(-1))
    # the dequantised rows are bf16 values (4 significant bits within bf16's exponent range) and the round trip is idempotent
    assert torch.equal(deq.to(torch.bfloat16).float(), deq)
    b2, s2 = quant_rule(deq.to(torch.bfloat16))
    assert torch.equal(dequant(b2, s2), deq)
    # -0.0 keeps its sign bit, the all-zero row has scale 1
    assert quant_rule(torch.full((1, 128), -0.0, dtype=torch.bfloat16))[0].unique().tolist() == [0x80]
    zb, zs = quant_rule(torch.zeros(1, 128, dtype=torch.bfloat16))
    assert zb.unique().tolist() == [0] and zs.tolist() == [1.0]
    # the error of an element is at most half an fp8 ulp at the top binade: 16 (the spacing at 256 ... 448 is 32), times the scale
    err = (deq - x.float()).abs().amax(-1).double()
    assert bool((err <= scale.double() * 16.0).all())


# ------------------------------------------------------------------------------------------------ C ABI
def test_entries_are_wired():
    header = open(os.path.join(ROOT, "include", "evo_mi355x.h")).read()
    for name in ENTRIES:
        assert name in _build.EXPORTS and name in evo_ops._SIGNATURES and re.search(r"\bint\s+" + name + r"\s*\(", header), name
    assert int(re.search(r"#define EVO_ABI_VERSION (\d+)", header).group(1)) == evo_ops.ABI_VERSION >= 19
    lib = evo_ops.load_library()
    assert lib.evo_abi_version() == evo_ops.ABI_VERSION
    assert Backend.OPTIONAL["kv_fp8"] == ("kv_quant_fp8", "rope_append_decode_fp8", "attention_decode_fp8")
    for meth in Backend.OPTIONAL["kv_fp8"]:
        assert hasattr(evo_ops.HipOps, meth), meth
    assert any(p.name == "kv_fp8.hip" for p in _build.sources())
    assert InferenceParams(max_seqlen=8, max_batch_size=1).kv_dtype == "bf16"


ONE = ctypes.c_void_p(16)                                             # non-null, 16-byte aligned, never dereferenced
F = ctypes.c_float
CACHE_OK = dict(d_sb=1 << 20, d_st=512, d_sw=256, d_sh=128, s_sb=4096, s_sw=2048, s_sh=1024)
CACHE_NAMES = list(CACHE_OK)
CACHE_BAD = [dict(d_sb=(1 << 20) + 8), dict(d_st=520), dict(d_sw=264), dict(d_sh=136), dict(d_st=64), dict(d_sw=0), dict(d_sh=0), dict(d_sb=-16),
             dict(s_sw=0), dict(s_sh=0), dict(s_sb=-1)]


def _caller(name, names, ok):
    f = getattr(evo_ops.load_library(), name)
    assert list(ok) == names and len(evo_ops._SIGNATURES[name][0]) == len(names)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return f(*[a[n] for n in names])
    return call


def test_kv_quant_refuses_before_any_launch():
    names = ["k", "v", "kv_data", "kv_scale", "B", "T", "H", "t0", "cap", "k_sb", "k_st", "k_sh", "v_sb", "v_st", "v_sh"] + CACHE_NAMES + ["stream"]
    ok = dict(k=ONE, v=ONE, kv_data=ONE, kv_scale=ONE, B=2, T=3, H=2, t0=1, cap=4, k_sb=2304, k_st=768, k_sh=128, v_sb=2304, v_st=768, v_sh=128,
              **CACHE_OK, stream=None)
    call = _caller("evo_kv_quant_fp8", names, ok)
    for n in ("k", "v", "kv_data", "kv_scale"):
        assert call(**{n: None}) == -1, n
    for n in ("k", "v", "kv_data"):
        assert call(**{n: ctypes.c_void_p(8)}) == -1 and call(**{n: ctypes.c_void_p(24)}) == -1, n
    assert call(kv_scale=ctypes.c_void_p(18)) == -1
    for kw in (dict(B=0), dict(T=0), dict(H=0), dict(B=-1), dict(t0=-1), dict(cap=0), dict(t0=2), dict(T=4, t0=1), dict(cap=3), dict(H=65536),
               dict(B=65536)):
        assert call(**kw) == -1, kw
    for n in ("k_sb", "k_st", "k_sh", "v_sb", "v_st", "v_sh"):
        assert call(**{n: ok[n] + 4}) == -1, n
    for kw in CACHE_BAD:
        assert call(**kw) == -1, kw


def test_rope_append_refuses_before_any_launch():
    names = ["qkv", "kv_data", "kv_scale", "pos", "inv_freq", "scaling", "B", "H", "hd"] + CACHE_NAMES + ["q_scale", "stream"]
    ok = dict(qkv=ONE, kv_data=ONE, kv_scale=ONE, pos=ONE, inv_freq=ONE, scaling=F(1.0), B=2, H=2, hd=128, **CACHE_OK, q_scale=F(1.0), stream=None)
    call = _caller("evo_rope_append_decode_fp8", names, ok)
    for n in ("qkv", "kv_data", "kv_scale", "pos", "inv_freq"):
        assert call(**{n: None}) == -1, n
    for n in ("qkv", "kv_data"):
        assert call(**{n: ctypes.c_void_p(8)}) == -1, n
    assert call(pos=ctypes.c_void_p(20)) == -1 and call(inv_freq=ctypes.c_void_p(18)) == -1 and call(kv_scale=ctypes.c_void_p(18)) == -1
    for kw in (dict(B=0), dict(H=0), dict(hd=64), dict(hd=256), dict(hd=0), dict(scaling=F(0.0)), dict(scaling=F(-1.0)), dict(q_scale=F(0.0)),
               dict(q_scale=F(float("nan"))), dict(scaling=F(float("nan")))):
        assert call(**kw) == -1, kw
    for kw in CACHE_BAD:
        assert call(**kw) == -1, kw


def test_attn_decode_refuses_before_any_launch():
    names = ["q", "kv_data", "kv_scale", "o", "B", "H", "Tk", "q_sb", "q_sh"] + CACHE_NAMES + ["dyn_pos", "part_o", "part_ml", "n_splits",
                                                                                                "softmax_scale", "stream"]
    ok = dict(q=ONE, kv_data=ONE, kv_scale=ONE, o=ONE, B=2, H=2, Tk=8, q_sb=768, q_sh=128, **CACHE_OK, dyn_pos=None, part_o=ONE, part_ml=ONE,
              n_splits=4, softmax_scale=F(0.0), stream=None)
    call = _caller("evo_attn_decode_fp8", names, ok)
    for n in ("q", "kv_data", "kv_scale", "o", "part_o", "part_ml"):
        assert call(**{n: None}) == -1, n
    for n in ("q", "kv_data", "o", "part_o"):
        assert call(**{n: ctypes.c_void_p(8)}) == -1, n
    assert call(dyn_pos=ctypes.c_void_p(20)) == -1 and call(kv_scale=ctypes.c_void_p(18)) == -1 and call(part_ml=ctypes.c_void_p(18)) == -1
    for kw in (dict(B=0), dict(H=0), dict(Tk=0), dict(n_splits=0), dict(n_splits=1025), dict(H=65536), dict(B=65536), dict(q_sb=772),
               dict(q_sh=132)):
        assert call(**kw) == -1, kw
    for kw in CACHE_BAD:
        assert call(**kw) == -1, kw
    # the streaming form addresses keys with 32-bit byte offsets and has no second form: Tk * d_st at or beyond 2^32 - 1 is refused
    assert call(Tk=1 << 19, d_st=8192) == -1                          # 2^32
    assert call(Tk=(1 << 32) // 8192 - 1, d_st=8192 + 16) == -1       # just beyond
    assert call(Tk=1 << 40, d_st=8192) == -1


# ------------------------------------------------------------------------------------------------ the backend, from the rule
class Fp8OracleOps(RaggedOracleOps):
    """+ the optional group "kv_fp8", written from the rule."""

    def __init__(self, act=torch.float64):
        super().__init__(act)
        self.fp8_calls = {"quant": 0, "append": 0, "decode": 0}

    def kv_quant_fp8(self, k, v, kv, t0=0):
        self.fp8_calls["quant"] += 1
        B, T = k.shape[:2]
        for w, x in enumerate((k, v)):
            byts, scale = quant_rule(x)
            kv.data[:B, t0:t0 + T, w] = byts
            kv.scale[:B, w, :, t0:t0 + T] = scale.permute(0, 2, 1)

    def rope_append_decode_fp8(self, qkv, kv, pos, inv_freq, scaling, q_scale=1.0):
        assert q_scale == 1.0
        self.fp8_calls["append"] += 1
        B, _, _, H, hd = qkv.shape
        t = pos.to(torch.float32)
        if scaling != 1.0:
            t = t / scaling
        freqs = torch.outer(t, inv_freq)
        self.rope_(qkv.view(1, B, 3, H, hd), torch.cos(freqs).to(torch.bfloat16).float(), torch.sin(freqs).to(torch.bfloat16).float())
        for b in range(B):
            one = Fp8KV(kv.data[b:b + 1], kv.scale[b:b + 1])
            Fp8OracleOps.kv_quant_fp8(self, qkv[b:b + 1, :, 1], qkv[b:b + 1, :, 2], one, t0=int(pos[b]))
            self.fp8_calls["quant"] -= 1

    def attention_decode_fp8(self, q, kv, pos=None, n_keys=None, n_splits=None, prescaled=False):
        self.fp8_calls["decode"] += 1
        B = q.shape[0]
        deq = Fp8KV(kv.data[:B], kv.scale[:B]).dequantize().double()
        k, v = deq[:, :, 0], deq[:, :, 1]
        if pos is None:
            n = k.shape[1] if n_keys is None else n_keys
            return self.attention_decode(q, k[:, :n], v[:, :n])
        return self.attention_decode(q, k, v, pos=pos)


def _model(ops):
    from oracle.stripedhyena_ref import RefConfig, make_synthetic_state_dict
    from evo_amd.sh.model import StripedHyena
    sd = make_synthetic_state_dict(RefConfig.from_dict(SMALL), seed=3)
    m = StripedHyena(dict(SMALL), ops=ops)
    if ops.act == torch.float64:
        sd = {k: (v.double() if v.dtype == torch.bfloat16 else v) for k, v in sd.items()}
    m.load_state_dict(sd)
    return m


@pytest.fixture(scope="module")
def small():
    return _model(Fp8OracleOps(torch.float64))


N_TOK, N_SPP = 5, 2


@pytest.fixture(scope="module")
def one_job_loop(small):
    """Every prompt alone: a cached prefill on an FP8 cache, then greedy single-token steps at a scalar offset -> [(ids, logits)]."""
    out = []
    with torch.inference_mode():
        for p in PROMPTS:
            ids = torch.tensor([list(p.encode())])
            ipd = small.initialize_inference_params()
            ipd["mha"].kv_dtype = "fp8"
            ipd["mha"].max_seqlen = ids.shape[1] + N_TOK
            logits, ipd = small(ids, inference_params_dict=ipd)
            assert isinstance(ipd["mha"].key_value_memory_dict[small.attn_layer_idxs[0]], Fp8KV)
            toks, rows, off = [], [], ids.shape[1]
            for _ in range(N_TOK):
                rows.append(logits[0, -1].float())
                toks.append(int(rows[-1].argmax()))
                ipd["mha"].seqlen_offset = ipd["hyena"].seqlen_offset = off
                logits, ipd = small(torch.tensor([[toks[-1]]]), inference_params_dict=ipd)
                off += 1
            out.append((toks, torch.stack(rows)))
    return out


@pytest.mark.parametrize("prefill_batch", [1, 4])
@pytest.mark.parametrize("n_slots", [3, 4])
def test_fp8_pool_equals_the_one_job_loop(small, one_job_loop, n_slots, prefill_batch):
    small.ops.fp8_calls = {"quant": 0, "append": 0, "decode": 0}
    pool = DecodePool(small, TOK, n_slots=n_slots, top_k=1, top_p=1.0, temperature=0.0, device="cpu", kv_dtype="fp8", prefill_batch=prefill_batch)
    seqs, scores, owner = pool.generate(PROMPTS, n_tokens=N_TOK, n_sample_per_prompt=N_SPP)
    assert owner == [pi for pi in range(len(PROMPTS)) for _ in range(N_SPP)]
    for j, pi in enumerate(owner):
        toks, rows = one_job_loop[pi]
        assert pool.last_ids[j].tolist() == toks and seqs[j] == "".join(chr(t) for t in toks), j
        # fp64 arithmetic on identical cached bytes: only the summation order of a batched step differs (tests/test_ragged_prefill_host.py)
        err, top = float((pool.last_logits[j].double() - rows.double()).abs().max()), float(rows.abs().max())
        assert err <= 1e-6 * top, (j, err, top)
    calls = small.ops.fp8_calls
    # every step appends and attends once (one attention layer); every prefill stores once and reads nothing back
    assert calls["append"] == calls["decode"] == pool.stats["steps"] > 0 and calls["quant"] == pool.stats["prefills"]
    assert (pool.stats["prefills"] == len(PROMPTS)) == (prefill_batch == 1) and pool.ipd["mha"].kv_dtype == "fp8"
    for kv in pool.ipd["mha"].key_value_memory_dict.values():
        assert isinstance(kv, Fp8KV) and kv.data.dtype == torch.uint8 and kv.scale.dtype == torch.float32
        assert tuple(kv.scale.shape) == (n_slots, 2, small.num_heads, kv.data.shape[1])


def test_kv_bytes_are_reported_and_about_half(small):
    cap = 96
    fp8 = DecodePool(small, TOK, n_slots=3, device="cpu", kv_dtype="fp8")
    fp8._allocate(cap)
    bf16_model = _model(Fp8OracleOps(torch.bfloat16))                  # (the fp64 oracle model would hold an fp64 cache)
    bf = DecodePool(bf16_model, TOK, n_slots=3, device="cpu")
    bf._allocate(cap)
    H, hd, L = small.num_heads, small.head_dim, len(small.attn_layer_idxs)
    assert hd == 128 and bf.capacity == fp8.capacity == cap
    assert bf.stats["kv_bytes"] == 3 * cap * 2 * H * hd * 2 * L
    assert fp8.stats["kv_bytes"] * 256 == bf.stats["kv_bytes"] * (128 + 4)
    # growing copies both tensors of a layer
    i = small.attn_layer_idxs[0]
    kv = fp8.ipd["mha"].key_value_memory_dict[i]
    kv.data.random_(0, 256)
    kv.scale.uniform_(0.5, 2.0)
    fp8._allocate(3 * cap)
    new = fp8.ipd["mha"].key_value_memory_dict[i]
    assert new is not kv and new.shape[1] >= 3 * cap and torch.equal(new.data[:, :cap], kv.data) and torch.equal(new.scale[..., :cap], kv.scale)
    assert fp8.stats["kv_bytes"] == new.nbytes() * L


def test_generator_runs_on_an_fp8_cache(small, one_job_loop):
    p = PROMPTS[1]
    gen = Generator(small, TOK, top_k=1, kv_dtype="fp8")
    ids, logits, ipd = gen.generate("cpu", input_string=p, num_tokens=N_TOK, print_generation=False)
    toks, rows = one_job_loop[1]
    assert ids[0].tolist() == toks and torch.equal(logits[0], rows)
    kv = ipd["mha"].key_value_memory_dict[small.attn_layer_idxs[0]]
    assert isinstance(kv, Fp8KV) and ipd["mha"].kv_dtype == "fp8" and kv.shape[1] >= len(p) + N_TOK - 1
    # the reference's schedule (a short prefill, then the rest of the prompt token by token) feeds single tokens: it keeps working
    ids2, _, _ = gen.generate("cpu", input_string=PROMPTS[0], num_tokens=2, force_prompt_threshold=7, print_generation=False)
    assert ids2[0].tolist() == one_job_loop[0][0][:2]
    # the default is untouched
    _, _, ipd = Generator(small, TOK, top_k=1).generate("cpu", input_string=p, num_tokens=2, print_generation=False)
    assert ipd["mha"].kv_dtype == "bf16" and isinstance(ipd["mha"].key_value_memory_dict[small.attn_layer_idxs[0]], torch.Tensor)


def test_what_is_refused(small):
    from evo_amd.sh.cache import SharedPrefix
    with pytest.raises(ValueError, match="kv_dtype"):
        DecodePool(small, TOK, n_slots=2, device="cpu", kv_dtype="fp16")
    with pytest.raises(ValueError, match="kv_dtype"):
        Generator(small, TOK, kv_dtype="int8")
    with pytest.raises(ValueError, match="kv_dtype"):
        sample_many(PROMPTS[:1], small, TOK, n_tokens=1, device="cpu", kv_dtype="e5m2")
    with pytest.raises(ValueError, match="kv_dtype"):
        small.prefill_ragged(torch.zeros(1, 4, dtype=torch.int64), [4], kv_dtype="fp4")
    with pytest.raises(ValueError, match="share_prompt_kv"):
        DecodePool(small, TOK, n_slots=2, device="cpu", kv_dtype="fp8", share_prompt_kv=True)
    # a backend without the group
    plain = _model(RaggedOracleOps(torch.float64))
    assert not plain.ops.supports("kv_fp8") and small.ops.supports("kv_fp8")
    with pytest.raises(RuntimeError, match="kv_fp8"):
        DecodePool(plain, TOK, n_slots=2, device="cpu", kv_dtype="fp8")
    with pytest.raises(RuntimeError, match="kv_fp8"):
        Generator(plain, TOK, kv_dtype="fp8")
    ids = torch.tensor([list(PROMPTS[1].encode())])
    ipd = plain.initialize_inference_params()
    ipd["mha"].kv_dtype = "fp8"
    with pytest.raises(RuntimeError, match="kv_fp8"):
        plain(ids, inference_params_dict=ipd)
    # a resumed multi-token prefill on an FP8 cache
    ipd = small.initialize_inference_params()
    ipd["mha"].kv_dtype = "fp8"
    with torch.inference_mode():
        _, ipd = small(ids, inference_params_dict=ipd)
        ipd["mha"].seqlen_offset = ipd["hyena"].seqlen_offset = ids.shape[1]
        with pytest.raises(ValueError, match="resumed multi-token prefill"):
            small(ids[:, :3], inference_params_dict=ipd)
    # shared_prefix and prompt_store
    from evo_amd.sh.cache import PromptStore
    for field, value in (("shared_prefix", SharedPrefix()), ("prompt_store", PromptStore())):
        ipd = small.initialize_inference_params()
        ipd["mha"].kv_dtype = "fp8"
        setattr(ipd["mha"], field, value)
        with pytest.raises(ValueError, match=field), torch.inference_mode():
            small(ids, inference_params_dict=ipd)
    # an unknown format on the record itself
    ipd = small.initialize_inference_params()
    ipd["mha"].kv_dtype = "fp4"
    with pytest.raises(ValueError, match="kv_dtype"), torch.inference_mode():
        small(ids, inference_params_dict=ipd)


def test_the_clis_take_the_option():
    for script, flag in (("sample_many.py", "--kv-dtype"), ("generate.py", "--kv-dtype")):
        text = open(os.path.join(ROOT, "scripts", script)).read()
        assert flag in text and "kv_dtype" in text, script


# ------------------------------------------------------------------------------------------------ resources
@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_fp8_kernels_need_no_scratch():
    meta = _metadata("kv_fp8.hip")
    kernels = {k: r for k, r in meta.items() if any(n in k for n in ("kv_quant_fp8_kernel", "rope_append_decode_fp8_kernel", "attn_decode_fp8_kernel"))}
    assert len(kernels) == 3 == len(meta), sorted(meta)
    for name, r in kernels.items():
        assert r["scratch"] == 0 and r["spill"] == 0 and r["sgpr_spill"] == 0 and r["lds"] == 0, (name, r)
    attn = next(r for k, r in kernels.items() if "attn_decode_fp8_kernel" in k)
    assert attn["vgpr"] <= 256, attn                                  # two waves per SIMD, as the bf16 streaming kernel
