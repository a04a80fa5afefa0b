"""GPU (-m gpu): every entry point of include/evo_mi355x.h -- every kernel instantiation behind it -- inside a poisoned arena.

The parity suite pins VALUES; this module pins MEMORY BEHAVIOUR.  Each case is one call of the binding run twice (tests/arena.py
run_in_arena): on fresh allocations on the current stream, and with every operand -- and every output / workspace the binding
allocates itself -- carved out of one 0xFF-filled tensor at an address that is 16 (mod 32) (integer vectors: 8 (mod 16), the weakest
alignment the model's call sites produce and all the header asks of them), between guard bands of >= 256 rows and
>= 64 KiB, on a side stream behind a multi-millisecond filler.  The two runs must agree bit for bit (returned tensors and every
operand; read-only operands unchanged) and no band may change.  A store past a ragged tile, a load past the end that reaches a sum,
an operand that quietly needs more than 16 bytes of alignment, a launch / pre-pass / memset on the wrong stream: each one fails here.

Every case names the entry points it must reach; a spy on the library handle asserts that it did, and the last test walks
evo_amd.ops._SIGNATURES so that a kernel added later cannot skip the arena.  Only contract-legal calls; shapes small or medium."""
import math

import pytest
import torch

import evo_amd.ops as evo_ops
from arena import run_in_arena

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
COVERED = set()


def covers(*names):
    """Declares (at import time) the entry points a case reaches; _run asserts at run time that the library was really called."""
    COVERED.update(names)

    def deco(f):
        f.entry_points = names
        return f
    return deco


class _Spy:
    def __init__(self, lib):
        self._lib = lib
        self.called = set()

    def __getattr__(self, name):
        self.called.add(name)
        return getattr(self._lib, name)


def _ops():
    return evo_ops.default_ops()


def _run(fn, inputs, inout=(), expect=(), **kw):
    ops = _ops()
    lib = ops.lib
    spy = _Spy(lib)
    ops.lib = spy
    try:
        run = run_in_arena(fn, inputs, inout=inout, module=evo_ops, release=ops.release_workspaces, **kw)
    finally:
        ops.lib = lib
    missing = set(expect) - spy.called
    assert not missing, f"the case never reached {sorted(missing)} (called: {sorted(spy.called)})"
    return run


def gen(seed):
    return torch.Generator(device=DEV).manual_seed(seed)


def rnd(shape, g, scale=1.0, dtype=BF):
    return (torch.randn(*shape, device=DEV, generator=g) * scale).to(dtype)


def poisoned(shape, dtype):
    t = torch.empty(shape, dtype=dtype, device=DEV)
    t.view(-1).view(torch.uint8).fill_(0xFF)
    return t


def is_poison(t):
    t = torch.view_as_real(t) if t.is_complex() else t
    return bool((t.contiguous().view(-1).view(torch.uint8) == 0xFF).all())


# ------------------------------------------------------------------------------------------------ the persistent dense layer (csrc/gemm.hip)
MFMA_SHAPES = [(9, 256, 64),                 # a single ragged tile
               (257, 512, 128), (300, 768, 192), (511, 512, 128),      # M % 256 in {1, 44, 255}, several N tiles; K = 128 / 192: the fetch cursor changes tile every 2 / 3 stages
               (8192 + 77, 4096, 128)]       # more tiles than workgroups, the ragged tile mid-list


@covers("evo_linear_mfma_bf16")
@pytest.mark.parametrize("bias,res", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("M,N,K", MFMA_SHAPES)
def test_linear_mfma(M, N, K, bias, res):
    ops, g = _ops(), gen(M + N + K)
    inp = {"x": rnd((M, K), g), "w": rnd((N, K), g, K ** -0.5)}
    if bias:
        inp["b"] = rnd((N,), g)
    if res:
        inp["r"] = rnd((M, N), g)
    _run(lambda x, w, b=None, r=None: ops.linear_mfma(x, w, b, r), inp, inout=["r"] if res else [], expect=["evo_linear_mfma_bf16"])


def _blocked(y, ops):
    M, K = y.shape
    nrb = (M + 127) // 128
    pad = torch.zeros(nrb * 128, K, dtype=BF, device=DEV)
    pad[:M] = y
    return pad.view(nrb, 128, K // 16, 16).permute(0, 2, 1, 3).contiguous()


@covers("evo_linear_xblk_mfma_bf16", "evo_linear_xblk_mfma_nf_bf16", "evo_rms_finalize_f32")
@pytest.mark.parametrize("stats", [False, True])
@pytest.mark.parametrize("bias", [False, True])
def test_linear_on_blocked_y_with_a_partly_filled_last_block(stats, bias):
    """768 + 200 rows: the blocked launch takes 768, the last 128-row block of y_blk is partly filled and goes row-major through the ordinary
    dense layer into the adjacent rows of the same residual; with `stats` the partial sums `ss` and `rstd` are carved too."""
    ops, g = _ops(), gen(41)
    M, N, K = 768 + 200, 512, 256
    inp = {"res": rnd((M, N), g), "y_blk": _blocked(rnd((M, K), g), ops), "w": rnd((N, K), g, K ** -0.5)}
    if bias:
        inp["b"] = rnd((N,), g)
    if stats:
        fn = lambda res, y_blk, w, b=None: ops.linear_residual_yblk_stats_(res, y_blk, w, b, 1e-6)[:M]     # (rstd rows >= M are never written)
        _run(fn, inp, inout=["res"], expect=["evo_linear_xblk_mfma_nf_bf16", "evo_rms_finalize_f32", "evo_linear_mfma_bf16"])
    else:
        _run(lambda res, y_blk, w, b=None: ops.linear_residual_yblk_(res, y_blk, w, bias=b), inp, inout=["res"],
             expect=["evo_linear_xblk_mfma_bf16", "evo_linear_mfma_bf16"])


@covers("evo_linear_mfma_nf_bf16", "evo_rms_finalize_f32", "evo_linear_small_m_bf16")
@pytest.mark.parametrize("M", [1024 + 1, 1024 + 16, 1024 + 44])
@pytest.mark.parametrize("bias", [False, True])
def test_stream_writing_dense_layer_with_sumsq(M, bias):
    """The `sumsq` form: M with a 1..16-row sliver -- the main launch and the weight-streaming launch write adjacent rows of one tensor --
    and M % 256 = 44 (one ragged tile, no sliver)."""
    ops, g = _ops(), gen(M)
    N, K = 512, 256
    inp = {"res": rnd((M, N), g, 3.0), "x": rnd((M, K), g), "w": rnd((N, K), g, K ** -0.5)}
    if bias:
        inp["b"] = rnd((N,), g)
    sliver = 1 <= M % 256 <= 16
    _run(lambda res, x, w, b=None: ops.linear_residual_stats_(res, x, w, b, 1e-6)[:M], inp, inout=["res"],
         expect=["evo_linear_mfma_nf_bf16", "evo_rms_finalize_f32"] + (["evo_linear_small_m_bf16"] if sliver else []))


@covers("evo_linear_mfma_nf_bf16", "evo_rms_finalize_f32")
@pytest.mark.parametrize("M", [1024 + 3, 1024 + 16, 700])
def test_dense_layer_with_row_scale(M):
    ops, g = _ops(), gen(M + 1)
    N, K = 768, 256
    inp = {"x": rnd((M, K), g, 2.0), "w": rnd((N, K), g, K ** -0.5), "b": rnd((N,), g), "scale": (1 + 0.1 * torch.randn(K, device=DEV, generator=g)).to(BF)}

    def fn(x, w, b, scale):
        rstd = ops.rms_finalize(None, x, 0, 1e-6)
        return rstd[:M], ops.linear_rs(x, rstd, ops.fold_norm_scale(w, scale), b, w, scale, 1e-6)
    _run(fn, inp, expect=["evo_linear_mfma_nf_bf16", "evo_rms_finalize_f32"])


@covers("evo_mlp_gate_mfma_bf16", "evo_mlp_gate_mfma_nf_bf16", "evo_mlp_gate_small_m_bf16")
@pytest.mark.parametrize("nf", [False, True])
@pytest.mark.parametrize("M,I,K", [(700, 256, 192), (4096 + 8, 128, 256)])
def test_gated_dense_layer(M, I, K, nf):
    ops, g = _ops(), gen(M + I + K)
    inp = {"x": rnd((M, K), g), "w12": rnd((2 * I, K), g, K ** -0.5)}
    if nf:
        inp["scale"] = (1 + 0.1 * torch.randn(K, device=DEV, generator=g)).to(BF)

        def fn(x, w12, scale):
            rstd = ops.rms_finalize(None, x, 0, 1e-6)
            return ops.mlp_gate_rs(x, rstd, ops.pack_gate_weights(ops.fold_norm_scale(w12, scale)), w12, scale, 1e-6)
        _run(fn, inp, expect=["evo_mlp_gate_mfma_nf_bf16"])
    else:
        _run(lambda x, w12: ops.mlp_gate(x, w12, w12g=ops.pack_gate_weights(w12)), inp,
             expect=["evo_mlp_gate_mfma_bf16"] + (["evo_mlp_gate_small_m_bf16"] if M % 256 == 8 else []))


# ------------------------------------------------------------------------------------------------ z^T producers
@covers("evo_rmsnorm_rows_bf16", "evo_linear_t_mfma_bf16", "evo_linear_small_m_bf16")
@pytest.mark.parametrize("bias", [False, True])
@pytest.mark.parametrize("B,T", [(2, 513), (3, 1025), (2, 1026), (3, 1003)])       # tail form with 1 / 1 / 2 tail tokens; the padded form
def test_zt_producers_both_forms(B, T, bias):
    """Pad rows of xp and pad positions of z^T are INSIDE the tensors (zeros / what the projection makes of zeros: the same bits in both
    runs); the bands around them may not change.  xp is the binding's cached workspace: it is carved too and dropped with the context."""
    ops, g = _ops(), gen(B * T)
    D = 256
    Tm, Tp, Mp, r = ops.zt_layout(B, T)
    assert (r > 0) == (T != 1003) and ops.zt_shape_ok(B, T, 3 * D, D)
    inp = {"x": rnd((B * T, D), g), "scale": (1 + 0.1 * torch.randn(D, device=DEV, generator=g)).to(BF), "w": rnd((3 * D, D), g, D ** -0.5)}
    if bias:
        inp["b"] = rnd((3 * D,), g, 0.1)

    def fn(x, scale, w, b=None):
        xp = ops.rmsnorm_rows(x, scale, 1e-6, B, T)
        return xp, ops.linear_t(xp, w, b, B, T)
    _run(fn, inp, expect=["evo_rmsnorm_rows_bf16", "evo_linear_t_mfma_bf16"] + (["evo_linear_small_m_bf16"] if r else []))


@covers("evo_linear_t_mfma_nf_bf16", "evo_rms_finalize_f32")
@pytest.mark.parametrize("tail", [True, False])
@pytest.mark.parametrize("B,T", [(2, 513), (3, 1025), (4, 512)])                   # tail form (the stream's rows remapped); plain form without a pad position
def test_zt_from_the_stream_rows_with_row_scale(B, T, tail):
    ops, g = _ops(), gen(B * T + 7)
    D = 256
    assert ops.zt_stream_rows_ok(B, T)
    inp = {"x": rnd((B * T, D), g, 2.0), "scale": (1 + 0.1 * torch.randn(D, device=DEV, generator=g)).to(BF), "w": rnd((3 * D, D), g, D ** -0.5),
           "b": rnd((3 * D,), g, 0.1)}

    def fn(x, scale, w, b):
        rstd = ops.rms_finalize(None, x, 0, 1e-6)
        return ops.linear_t_rs(x, rstd, ops.fold_norm_scale(w, scale), b, w, scale, 1e-6, B, T, tail=tail)
    _run(fn, inp, expect=["evo_linear_t_mfma_nf_bf16", "evo_rms_finalize_f32"])


# ------------------------------------------------------------------------------------------------ weight-streaming launches (csrc/gemv.hip)
SMALL_M = ([(M, 512, 256) for M in (1, 4,            # dot2
                                    5, 16,           # skinny_mfma
                                    17, 64)]         # SPLITK + reduce: the workspace is carved
           + [(M, 8200, 256) for M in (5, 64)]       # skinny_nw, ragged last n tile
           + [(M, 37, 264) for M in (1, 4, 8)])      # K % 32 != 0, rows of 74 bytes


@covers("evo_linear_small_m_bf16")
@pytest.mark.parametrize("mode", ["plain", "bias", "residual"])
@pytest.mark.parametrize("M,N,K", SMALL_M)
def test_linear_small_m(M, N, K, mode):
    ops, g = _ops(), gen(M * 1000 + N + K)
    inp = {"x": rnd((M, K), g), "w": rnd((N, K), g, 0.05)}
    assert ops._use_small_m(inp["x"], inp["w"])
    if mode == "bias":
        inp["b"] = rnd((N,), g)
    if mode == "residual":
        inp["r"] = rnd((M, N), g)
    _run(lambda x, w, b=None, r=None: ops._linear_small_m(x, w, b, r), inp, inout=["r"] if mode == "residual" else [], expect=["evo_linear_small_m_bf16"])


@covers("evo_norm_linear_small_m_bf16")
@pytest.mark.parametrize("M,N,K", [(1, 4104, 264), (4, 4104, 264), (8, 4352, 4096)])
def test_norm_linear_small_m(M, N, K):
    ops, g = _ops(), gen(M * 13 + N + K)
    inp = {"x": rnd((M, K), g, 3.0), "scale": (1 + 0.1 * torch.randn(K, device=DEV, generator=g)).to(BF), "w": rnd((N, K), g, K ** -0.5), "b": rnd((N,), g)}
    _run(lambda x, scale, w, b: ops.norm_linear(x, scale, 1e-6, w, b), inp, expect=["evo_norm_linear_small_m_bf16"])


@covers("evo_mlp_gate_small_m_bf16")
@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("M,I,K", [(1, 64, 264), (4, 64, 264),          # dot2
                                   (5, 128, 256), (64, 128, 256)])      # MFMA with the gate in its epilogue
def test_mlp_gate_small_m(M, I, K, grouped):
    ops, g = _ops(), gen(M * 77 + I + K)
    inp = {"x": rnd((M, K), g), "w12": rnd((2 * I, K), g, 1.5 * K ** -0.5)}
    if grouped:
        inp["w12"] = ops.pack_gate_weights(inp["w12"])
        _run(lambda x, w12: ops.mlp_gate(x, None, w12g=w12), inp, expect=["evo_mlp_gate_small_m_bf16"])
    else:
        _run(lambda x, w12: ops.mlp_gate(x, w12), inp, expect=["evo_mlp_gate_small_m_bf16"])


@covers("evo_norm_mlp_gate_small_m_bf16")
@pytest.mark.parametrize("grouped", [False, True])
@pytest.mark.parametrize("M,I,K", [(1, 64, 264), (4, 64, 264), (8, 64, 4096)])
def test_norm_mlp_gate_small_m(M, I, K, grouped):
    ops, g = _ops(), gen(M + I + K)
    inp = {"x": rnd((M, K), g, 2.0), "scale": (1 + 0.1 * torch.randn(K, device=DEV, generator=g)).to(BF), "w12": rnd((2 * I, K), g, 1.5 * K ** -0.5)}
    if grouped:
        inp["w12"] = ops.pack_gate_weights(inp["w12"])
        _run(lambda x, scale, w12: ops.mlp_gate(x, None, scale, 1e-6, w12g=w12), inp, expect=["evo_norm_mlp_gate_small_m_bf16"])
    else:
        _run(lambda x, scale, w12: ops.mlp_gate(x, w12, scale, 1e-6), inp, expect=["evo_norm_mlp_gate_small_m_bf16"])


def hyena_params(D, seed):
    g = gen(seed)
    fir_w = rnd((3 * D, 3), g, 0.3)
    fir_b = rnd((3 * D,), g, 0.1)
    one_minus = 10.0 ** (-5.0 + 4.0 * torch.rand(D, 8, device=DEV, generator=g))
    mag, ang = 1.0 - one_minus, (torch.rand(D, 8, device=DEV, generator=g) * 2 - 1) * math.pi
    poles = torch.stack([mag * torch.cos(ang), mag * torch.sin(ang)], -1).float().contiguous()
    res = (torch.randn(D, 8, 2, device=DEV, generator=g) * torch.sqrt(one_minus).unsqueeze(-1)).float().contiguous()
    dskip = rnd((D,), g, 0.5)
    return dict(fir_w=fir_w, fir_b=fir_b, poles=poles, residues=res, dskip=dskip)


def c64(shape, g):
    return torch.view_as_complex(torch.randn(*shape, 2, device=DEV, generator=g).contiguous())


@covers("evo_hyena_decode_fused_small_m")
@pytest.mark.parametrize("M,D,H", [(1, 512, 4), (4, 512, 4), (8, 4096, 32)])
def test_hyena_decode_fused_small_m(M, D, H):
    """fir_state / iir_state are in/out."""
    ops, g = _ops(), gen(M + D)
    inp = dict(hyena_params(D, 200 + M), x=rnd((M, D), g, 2.0), scale=(1 + 0.1 * torch.randn(D, device=DEV, generator=g)).to(BF),
               w=rnd((3 * D, D), g, D ** -0.5), b=rnd((3 * D,), g, 0.1), fs=rnd((M, 3 * D, 2), g), st=c64((M, D, 8), g))

    def fn(x, scale, w, b, fs, st, fir_w, fir_b, poles, residues, dskip):
        return ops.hyena_decode_fused(x, scale, 1e-6, w, b, fs, st, fir_w, fir_b, poles, residues, dskip, H)
    _run(fn, inp, inout=["fs", "st"], expect=["evo_hyena_decode_fused_small_m"])


# ------------------------------------------------------------------------------------------------ elementwise, scoring tail
@covers("evo_embed_bf16")
def test_embed():
    ops, g = _ops(), gen(0)
    ids = torch.randint(0, 512, (3, 17), device=DEV, generator=g)
    _run(lambda ids, w: ops.embed(ids, w), {"ids": ids, "w": rnd((512, 256), g)}, expect=["evo_embed_bf16"], align={"ids": 8})


@covers("evo_rmsnorm_bf16")
@pytest.mark.parametrize("with_bias", [False, True])
@pytest.mark.parametrize("M,D", [(5, 256), (37, 4096), (3, 1024), (2, 8192)])
def test_rmsnorm(M, D, with_bias):
    ops, g = _ops(), gen(2)
    inp = {"x": rnd((M, D), g, 3.0), "scale": (1 + 0.1 * torch.randn(D, device=DEV, generator=g)).to(BF)}
    if with_bias:
        inp["bias"] = rnd((D,), g)
    _run(lambda x, scale, bias=None: ops.rmsnorm(x, bias, scale, 1e-6), inp, inout=["x"] if with_bias else [], expect=["evo_rmsnorm_bf16"])


@covers("evo_rope_qk_bf16")
@pytest.mark.parametrize("q_scale", [1.0, None])
@pytest.mark.parametrize("B,T,H,hd", [(2, 19, 2, 128), (1, 5, 1, 64), (1, 300, 4, 128)])
def test_rope(B, T, H, hd, q_scale):
    ops, g = _ops(), gen(5)
    t = torch.arange(7, 7 + T, dtype=torch.float32, device=DEV)
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32, device=DEV) / hd))
    fr = torch.outer(t, inv)
    inp = {"qkv": rnd((B, T, 3, H, hd), g), "cos": torch.cos(fr).to(BF).float().contiguous(), "sin": torch.sin(fr).to(BF).float().contiguous()}
    qs = ops.attn_q_scale(hd) if q_scale is None else q_scale
    _run(lambda qkv, cos, sin: ops.rope_(qkv, cos, sin, q_scale=qs), inp, inout=["qkv"], expect=["evo_rope_qk_bf16"])


@covers("evo_gelu_gate_bf16")
@pytest.mark.parametrize("M,I", [(7, 64), (33, 10928)])
def test_gelu_gate(M, I):
    ops = _ops()
    _run(lambda gg: ops.gelu_gate(gg), {"gg": rnd((M, 2 * I), gen(6), 2.0)}, expect=["evo_gelu_gate_bf16"])


@covers("evo_logprob_entropy")
@pytest.mark.parametrize("dtype", [BF, torch.float32])
def test_logprob_entropy(dtype):
    ops, g = _ops(), gen(7)
    tgt = torch.randint(0, 512, (41,), device=DEV, generator=g)
    tgt[3] = -1
    _run(lambda logits, tgt: ops.logprob_entropy(logits, tgt, want_logprob=True, want_entropy=True),
         {"logits": rnd((41, 512), g, 4.0, dtype), "tgt": tgt}, expect=["evo_logprob_entropy"], align={"tgt": 8})


@covers("evo_unembed_logprob_bf16")
@pytest.mark.parametrize("M,K", [(70, 32), (70, 288), (63, 4096), (513, 256)])
def test_unembed_logprob(M, K):
    ops, g = _ops(), gen(30)
    tgt = torch.randint(0, 512, (M,), device=DEV, generator=g)
    tgt[M // 2] = -1
    inp = {"hid": rnd((M, K), g), "emb": rnd((512, K), g, 4.0 / math.sqrt(K)), "tgt": tgt}
    assert ops.unembed_logprob_ok(inp["hid"], inp["emb"])
    _run(lambda hid, emb, tgt: ops.unembed_logprob(hid, emb, tgt, want_logprob=True, want_entropy=True), inp, expect=["evo_unembed_logprob_bf16"], align={"tgt": 8})


@covers("evo_rope_append_decode_bf16")
@pytest.mark.parametrize("q_scale", [1.0, None])
def test_rope_append_decode_touches_one_cache_row_per_stream(q_scale):
    """B rows at scattered positions, including 0 and cap - 1; the cache starts as 0xFF and every row that is not (b, pos[b]) must still be."""
    ops, g = _ops(), gen(9)
    H, hd, cap = 2, 128, 40
    positions = [0, cap - 1, 17, 5, 38]
    B = len(positions)
    inv = 1.0 / (10000.0 ** (torch.arange(0, hd, 2, dtype=torch.float32, device=DEV) / hd))
    inp = {"qkv": rnd((B, 1, 3, H, hd), g), "kv": poisoned((B + 1, cap, 2, H, hd), BF), "pos": torch.tensor(positions, dtype=torch.int64, device=DEV),
           "inv": inv.contiguous()}
    qs = ops.attn_q_scale(hd) if q_scale is None else q_scale
    run = _run(lambda qkv, kv, pos, inv: ops.rope_append_decode(qkv, kv[:B], pos, inv, 16.0, q_scale=qs), inp, inout=["qkv", "kv"],
               expect=["evo_rope_append_decode_bf16"], align={"pos": 8})
    for kv in (run.inputs["kv"], run.fresh_inputs["kv"]):
        written = torch.zeros(B + 1, cap, dtype=torch.bool, device=DEV)
        written[torch.arange(B, device=DEV), inp["pos"]] = True
        rows = (kv.contiguous().view(B + 1, cap, -1).view(torch.uint8) == 0xFF).all(-1)
        assert torch.equal(rows, ~written)
        assert torch.equal(kv[torch.arange(B, device=DEV), inp["pos"]][:, 0], run.inputs["qkv"][:, 0, 1])      # k appended as rotated


# ------------------------------------------------------------------------------------------------ Hyena operator
@covers("evo_hyena_seg_state", "evo_hyena_carry_scan", "evo_hyena_apply")
@pytest.mark.parametrize("B,T,seg", [(2, 301, 32), (1, 37, 8), (2, 513, None)])
def test_hyena_modal_prefill_with_mask_halo_and_carry_in(B, T, seg):
    """T not a multiple of the segment; `agg` and the end state land in the arena through the proxy."""
    ops, g = _ops(), gen(T)
    D, H = 256, 2
    mask = torch.ones(B, T, dtype=torch.uint8, device=DEV)
    mask[0, 0] = 0
    mask[0, 30:35] = 0
    mask[-1, T - 20:] = 0
    inp = dict(hyena_params(D, 40), z=rnd((B, T, 3 * D), g), halo=rnd((B, 2, 3 * D), g), s0=c64((B, D, 8), g), mask=mask)

    def fn(z, halo, s0, mask, fir_w, fir_b, poles, residues, dskip):
        y, st = ops.hyena_prefill(z, fir_w, fir_b, poles, residues, dskip, H, z_halo=halo, s0=s0, want_state=True, seg_len=seg, mask=mask)
        return y, st
    _run(fn, inp, expect=["evo_hyena_seg_state", "evo_hyena_carry_scan", "evo_hyena_apply"])


@covers("evo_hyena_seg_state", "evo_hyena_carry_scan", "evo_hyena_carry_add", "evo_hyena_apply")
def test_hyena_modal_two_stages():
    ops, g = _ops(), gen(77)
    B, T, D, H = 2, 301, 256, 2
    inp = dict(hyena_params(D, 41), z=rnd((B, T, 3 * D), g), halo=rnd((B, 2, 3 * D), g), s0=c64((B, D, 8), g))

    def fn(z, halo, s0, fir_w, fir_b, poles, residues, dskip):
        st1, s_end = ops.hyena_stage1(z, fir_w, fir_b, poles, H, z_halo=halo, seg_len=32)
        y = ops.hyena_stage2(z, fir_w, fir_b, poles, residues, dskip, H, st1, z_halo=halo, s0=s0)
        return s_end, y, st1[0]
    _run(fn, inp, expect=["evo_hyena_seg_state", "evo_hyena_carry_scan", "evo_hyena_carry_add", "evo_hyena_apply"])


@covers("evo_hyena_step")
@pytest.mark.parametrize("B", [1, 3])
def test_hyena_step(B):
    ops, g = _ops(), gen(18)
    D, H = 256, 2
    inp = dict(hyena_params(D, 18), z_t=rnd((B, 3 * D), g), fs=rnd((B, 3 * D, 2), g), st=c64((B, D, 8), g))
    _run(lambda z_t, fs, st, fir_w, fir_b, poles, residues, dskip: ops.hyena_step(z_t, fs, st, fir_w, fir_b, poles, residues, dskip, H), inp,
         inout=["fs", "st"], expect=["evo_hyena_step"])


def _ct_inputs(B, T, D, seed, b_total=None):
    from evo_amd.hyena_tables import mfma_operand_table
    ops, g = _ops(), gen(seed)
    prm = hyena_params(D, seed + 1)
    Bt = b_total or B
    z = rnd((Bt, T, 3 * D), g)
    return dict(zt=ops.zt_from_rows(z, Bt, T, float("nan")), fir_w=prm["fir_w"], fir_b=prm["fir_b"], poles=prm["poles"],
                table=mfma_operand_table(prm["poles"], prm["residues"], prm["dskip"]), halo=rnd((B, 2, 3 * D), g), s0=c64((B, D, 8), g))


@covers("evo_hyena_ct")
@pytest.mark.parametrize("carry", [False, True])
@pytest.mark.parametrize("B,T,D,H", [(2, 37, 128, 1), (2, 513, 256, 2), (3, 1003, 256, 2), (40, 300, 128, 1)])     # (40 x 300: more batch rows than row streams)
def test_hyena_ct_row_major_y_and_end_state(B, T, D, H, carry):
    ops = _ops()
    inp = _ct_inputs(B, T, D, 100 + T)

    def fn(zt, fir_w, fir_b, poles, table, halo, s0):
        kw = dict(z_halo=halo, s0=s0) if carry else {}
        return ops.hyena_ct(zt, B, T, fir_w, fir_b, table, H, want_state=True, poles=poles, **kw)
    _run(fn, inp, expect=["evo_hyena_ct"])


@covers("evo_hyena_ct")
@pytest.mark.parametrize("B,T,D,H", [(2, 513, 256, 2), (3, 300, 128, 1)])
def test_hyena_ct_blocked_y_behind_row0(B, T, D, H):
    """y_blk with y_row0 = 77: the 77 rows in front and the rows behind the last one (inside the last 128-row block) stay 0xFF."""
    ops = _ops()
    inp = _ct_inputs(B, T, D, 300 + T)
    rows = B * T + 77
    inp["y_blk"] = poisoned(((rows + 127) // 128, D // 16, 128, 16), BF)
    run = _run(lambda zt, fir_w, fir_b, poles, table, halo, s0, y_blk: ops.hyena_ct(zt, B, T, fir_w, fir_b, table, H, z_halo=halo, s0=s0, y_blk=y_blk, y_row0=77),
               inp, inout=["y_blk"], expect=["evo_hyena_ct"])
    yb = run.inputs["y_blk"]
    full = ops.yblk_to_rows(yb, yb.shape[0] * 128)
    assert is_poison(full[:77]) and is_poison(full[rows:]) and not bool(torch.isnan(full[77:rows].float()).any())


@covers("evo_hyena_ct")
@pytest.mark.parametrize("B,T,D,H", [(2, 513, 256, 2), (3, 1003, 256, 2), (2, 1024, 128, 1)])
def test_hyena_ct_state_only_writes_nothing_but_the_state(B, T, D, H):
    ops = _ops()
    inp = _ct_inputs(B, T, D, 500 + T)
    _run(lambda zt, fir_w, fir_b, poles, table, halo, s0: ops.hyena_ct(zt, B, T, fir_w, fir_b, table, H, z_halo=halo, s0=s0, poles=poles, state_only=True),
         inp, expect=["evo_hyena_ct"])


@covers("evo_hyena_ct")
@pytest.mark.parametrize("B,T,D,H", [(2, 513, 256, 2), (2, 1026, 128, 1)])
def test_hyena_ct_main_only_leaves_the_tail_rows_alone(B, T, D, H):
    """main_only (tail form): rows b T + Tm .. of y belong to the caller and must stay 0xFF; the rest and the state after token Tm - 1
    compare bit for bit."""
    ops = _ops()
    inp = _ct_inputs(B, T, D, 700 + T)
    Tm = ops.zt_layout(B, T)[0]
    keep = []

    def fn(zt, fir_w, fir_b, poles, table, halo, s0):
        y, st = ops.hyena_ct(zt, B, T, fir_w, fir_b, table, H, want_state=True, poles=poles, main_only=True)
        keep.append(y)
        return y[:, :Tm], st
    _run(fn, inp, expect=["evo_hyena_ct"])
    assert Tm < T and is_poison(keep[-1][:, Tm:]) and not bool(torch.isnan(keep[-1][:, :Tm].float()).any())


@covers("evo_hyena_ct")
@pytest.mark.parametrize("T", [700, 1026])
def test_hyena_ct_row_subrange(T):
    ops = _ops()
    B, D, H = 5, 256, 2
    inp = _ct_inputs(2, T, D, 900 + T, b_total=B)
    _run(lambda zt, fir_w, fir_b, poles, table, halo, s0: ops.hyena_ct(zt, 2, T, fir_w, fir_b, table, H, z_halo=halo, s0=s0, want_state=True, poles=poles,
                                                                      b_first=3, b_total=B), inp, expect=["evo_hyena_ct"])


# ------------------------------------------------------------------------------------------------ attention
@covers("evo_attn_fwd_causal_bf16")
@pytest.mark.parametrize("w64", [True, False])
@pytest.mark.parametrize("B,H,T", [(2, 2, 37), (1, 2, 128), (1, 2, 130), (1, 2, 513), (2, 1, 1000)])
def test_attention_on_the_thirds_of_a_packed_qkv(B, H, T, w64):
    """Tq <= 128: the decode-sized kernel; beyond: the 64-rows-per-wave kernel with its V^T pre-pass (`vt` carved) or, with attn_w64 = False,
    the 8-wave pipelined kernel.  q, k, v are strided views of one packed qkv."""
    ops = _ops()
    inp = {"qkv": rnd((B, T, 3, H, 128), gen(20 + T))}
    was = ops.attn_w64
    ops.attn_w64 = w64
    try:
        _run(lambda qkv: ops.attention(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], 0), inp, expect=["evo_attn_fwd_causal_bf16"])
    finally:
        ops.attn_w64 = was


@covers("evo_attn_fwd_causal_bf16")
@pytest.mark.parametrize("w64", [True, False])
@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("B,H,Tq,Tk,off", [(2, 2, 1, 300, 299), (1, 2, 64, 200, 136), (1, 1, 130, 700, 570), (1, 2, 513, 600, 87)])
def test_attention_against_a_kv_cache_with_slack(B, H, Tq, Tk, off, pre, w64):
    """Chunk continuation: k / v are views of a KV cache [B, Tk + 37, 2, H, 128] whose rows behind Tk hold 0xFF (NaN)."""
    ops, g = _ops(), gen(Tq + Tk)
    kv = poisoned((B, Tk + 37, 2, H, 128), BF)
    kv[:, :Tk] = rnd((B, Tk, 2, H, 128), g)
    inp = {"qkv": rnd((B, Tq, 3, H, 128), g, ops.attn_q_scale(128) if pre else 1.0), "kv": kv}
    was = ops.attn_w64
    ops.attn_w64 = w64
    try:
        _run(lambda qkv, kv: ops.attention(qkv[:, :, 0], kv[:, :Tk, 0], kv[:, :Tk, 1], off, prescaled=pre), inp, expect=["evo_attn_fwd_causal_bf16"])
    finally:
        ops.attn_w64 = was


@covers("evo_attn_decode_bf16")
@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("B,H,Tk,splits", [(2, 2, 1, None), (1, 2, 65, 3), (2, 2, 65, None), (1, 2, 96, 2), (2, 2, 96, None), (2, 3, 2048 + 33, None),
                                           (2, 3, 2048 + 33, 5)])
def test_attention_decode(B, H, Tk, splits, with_pos):
    """part_o / part_ml are carved; with `pos` the rows sit at different positions (the last one at Tk - 1) of the full-capacity view."""
    ops, g = _ops(), gen(Tk)
    inp = {"q": rnd((B, 1, H, 128), g), "kv": rnd((B, Tk + 37, 2, H, 128), g)}
    if with_pos:
        inp["pos"] = torch.tensor([max(0, Tk - 1 - 40 * (B - 1 - b)) for b in range(B)], dtype=torch.int64, device=DEV)
        _run(lambda q, kv, pos: ops.attention_decode(q, kv[:, :, 0], kv[:, :, 1], pos=pos, n_splits=splits), inp, expect=["evo_attn_decode_bf16"], align={"pos": 8})
    else:
        _run(lambda q, kv: ops.attention_decode(q, kv[:, :Tk, 0], kv[:, :Tk, 1], n_splits=splits), inp, expect=["evo_attn_decode_bf16"])


# ------------------------------------------------------------------------------------------------ pooling, sampling, probes
@covers("evo_pool_rows_bf16")
@pytest.mark.parametrize("norm", [False, True])
@pytest.mark.parametrize("mode", ["mean", "last"])
@pytest.mark.parametrize("D,ld", [(256, 256), (256, 264), (4096, 4096)])
def test_pool_rows_ragged_ranges(D, ld, mode, norm):
    """Ragged ranges incl. one row, the first and the last row of x; x a view with a row pitch > D; the strip workspace is carved."""
    ops, g = _ops(), gen(D + ld)
    M = 300
    inp = {"xp": rnd((M, ld), g), "ranges": torch.tensor([[0, 37], [37, 1], [38, 113], [151, 149], [299, 1]], dtype=torch.int64, device=DEV)}
    if norm:
        inp["scale"] = (1 + 0.1 * torch.randn(D, device=DEV, generator=g)).to(BF)
    _run(lambda xp, ranges, scale=None: ops.pool_rows(xp[:, :D], ranges, scale=scale, mode=mode), inp, expect=["evo_pool_rows_bf16"], align={"ranges": 8})


@covers("evo_sample_rows_f32")
@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("S,ld", [(5, 512), (33, 520)])
def test_sample_rows_with_histories_inactive_rows_and_a_row_pitch(S, ld, f32):
    """Per-row vectors carved at their ELEMENT's alignment (the decode pool passes one-element slices of its per-slot vectors: the header asks
    no more of them); inactive rows write nothing -- ids_out / logprob_out / histories start as 0xFF and those rows must still be."""
    ops, g = _ops(), gen(S)
    L = 4
    active = torch.ones(S, dtype=torch.bool, device=DEV)
    active[1::3] = False
    count = torch.arange(S, dtype=torch.int64, device=DEV) % (L + 2)              # (rows with count >= L record nothing)
    inp = {"lg": rnd((S, ld), g, 3.0, torch.float32 if f32 else BF), "top_k": torch.full((S,), 4, dtype=torch.int32, device=DEV),
           "top_p": torch.full((S,), 0.9, dtype=torch.float32, device=DEV), "temp": torch.full((S,), 0.7, dtype=torch.float32, device=DEV),
           "stream": torch.arange(S, dtype=torch.int64, device=DEV) * 3 + 1, "count": count, "active": active,
           "allow": ops.pack_allow_mask(torch.arange(512) % 3 != 0, DEV),
           "ids": poisoned((S,), torch.int64), "lp": poisoned((S,), torch.float32), "hist_ids": poisoned((S, L), torch.int64),
           "hist_logits": poisoned((S, L, 512), torch.float32)}
    inp["top_k"][0] = 1
    inp["top_k"][-1] = 0

    def fn(lg, top_k, top_p, temp, stream, count, active, allow, ids, lp, hist_ids, hist_logits):
        ops.sample_rows(lg[:, :512], top_k, top_p, temp, 1234, stream=stream, count=count, allow=allow, active=active, ids_out=ids, logprob_out=lp,
                        hist_ids=hist_ids, hist_logits=hist_logits)
    run = _run(fn, inp, inout=["count", "ids", "lp", "hist_ids", "hist_logits"], expect=["evo_sample_rows_f32"],
               align={"top_k": 4, "top_p": 4, "temp": 4, "stream": 8, "count": 8, "active": 1, "ids": 8, "lp": 4, "hist_ids": 8})
    got = run.inputs
    assert torch.equal(got["count"], count + active.long())
    for s in range(S):
        if not bool(active[s]):
            assert is_poison(got["ids"][s]) and is_poison(got["lp"][s]) and is_poison(got["hist_ids"][s]) and is_poison(got["hist_logits"][s])
        else:
            assert 0 <= int(got["ids"][s]) < 512 and int(got["ids"][s]) % 3 != 0
            for j in range(L):
                assert is_poison(got["hist_logits"][s, j]) == (j != int(count[s]))


@covers("evo_rms_finalize_f32")
@pytest.mark.parametrize("M,D", [(5, 256), (1027, 512)])
def test_rms_finalize_from_the_rows(M, D):
    ops = _ops()
    _run(lambda x: ops.rms_finalize(None, x, 0, 1e-6)[:M], {"x": rnd((M, D), gen(M), 2.0)}, expect=["evo_rms_finalize_f32"])


@covers("evo_probe_copy_f4", "evo_probe_mfma_bf16")
def test_probes():
    ops = _ops()
    n = 16 * 100003                                                     # (not a multiple of a workgroup's 4 KiB)
    src = torch.randint(0, 255, (n,), dtype=torch.uint8, device=DEV, generator=gen(1))

    def fn(src, dst, sink):
        evo_ops._check(ops.lib.evo_probe_copy_f4(src.data_ptr(), dst.data_ptr(), n, evo_ops._stream()), "evo_probe_copy_f4")
        evo_ops._check(ops.lib.evo_probe_mfma_bf16(sink.data_ptr(), 3, 4, evo_ops._stream()), "evo_probe_mfma_bf16")
    run = _run(fn, {"src": src, "dst": poisoned((n,), torch.uint8), "sink": poisoned((3 * 256,), torch.float32)}, inout=["dst", "sink"],
               expect=["evo_probe_copy_f4", "evo_probe_mfma_bf16"])
    assert torch.equal(run.inputs["dst"], src)


# ------------------------------------------------------------------------------------------------ the harness on the GPU, on stand-ins written in torch
def test_harness_catches_a_launch_on_another_stream_and_an_unwritten_row():
    """What tests/test_arena_host.py shows on a CPU arena, for the two ingredients only a GPU has: work enqueued on any stream but the
    caller's runs ahead of the filler and reads the poison; an output row nobody writes keeps it.  (Only in-range accesses: the
    out-of-range direction is shown by the CPU stand-ins alone.)"""
    from arena import ArenaError
    x = rnd((300, 64), gen(3))

    def on_the_default_stream(x):
        with torch.cuda.stream(torch.cuda.default_stream()):
            return x.float() * 2

    def last_row_unwritten(x):
        y = evo_ops.torch.empty(300, 64, dtype=BF, device=x.device)
        y[:299] = x[:299]
        return y
    with pytest.raises(ArenaError, match=r"returned tensor #0 .*first at \(0, 0\).*arena nan"):
        run_in_arena(on_the_default_stream, {"x": x}, module=evo_ops)
    run_in_arena(on_the_default_stream, {"x": x}, module=evo_ops, side_stream=False)         # the diagnosis switch: on the caller's stream it is fine
    with pytest.raises(ArenaError, match=r"returned tensor #0 .*64 of 19200 elements differ, first at \(299, 0\)"):
        run_in_arena(last_row_unwritten, {"x": x}, module=evo_ops)
    run_in_arena(lambda x: x.float() * 2, {"x": x}, module=evo_ops)
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ nobody skips the arena
def test_every_entry_point_is_named_by_a_case():
    missing = set(evo_ops._SIGNATURES) - {"evo_abi_version"} - COVERED
    assert not missing, f"entry points without an arena case: {sorted(missing)}"
