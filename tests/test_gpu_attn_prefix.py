"""GPU (-m gpu): causal attention over a shared prefix plus a private suffix (evo_attn_fwd_prefix_bf16, csrc/attn_w64.hip SEG).

Kernel vs the shipped entry: `ops.attention` (evo_attn_fwd_causal_bf16 with its V^T workspace) on the concatenated, batch-expanded
K / V with q_pos0 = P.  Tolerance ZERO: the two launches walk the same key tiles in the same order with the same arithmetic; a
mismatch means the trip diverged.  The cases put the seam between the segments inside the prologue's prefetch (P = 64), on the first
descriptor computed before the loop (P = 256: tile 4) and on the first one computed inside it (P = 320: tile 5); the suffix lengths
give a ragged last tile, a 1-row first query block and more than one block; (B, H) = (1, 8) takes the other block map.
Also against tests/gpu_ref64.causal_attention64 under the metric and bounds of
test_gpu_fulldepth.test_attention_h32_t8193_vs_eager_fp64 (worst head rel-L2 < 4e-3, worst |err| - 2^-7 |ref| < 2e-2).

The arena cases of the two new entries live here (tests/test_gpu_arena.py is not edited): `covers` registers them at import, as
tests/test_gpu_profile.py does."""
import ctypes

import pytest
import torch

from gpu_ref64 import causal_attention64
from test_gpu_arena import _run, covers, gen, poisoned, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
SLACK = 37          # cache rows behind the prefix: 0xFF (NaN) -- a load past P that reaches a sum shows


@pytest.fixture(scope="module")
def ops():
    from evo_amd.ops import HipOps
    return HipOps()


def _inputs(ops, B, H, P, Tq, pre):
    g = gen(1000 * B + 100 * H + P + Tq + int(pre))
    kv = poisoned((1, P + SLACK, 2, H, 128), BF)
    kv[:, :P] = rnd((1, P, 2, H, 128), g)
    qkv = rnd((B, Tq, 3, H, 128), g)                              # every batch row its own suffix
    if pre:
        qkv[:, :, 0] = (qkv[:, :, 0].float() * ops.attn_q_scale(128)).to(BF)
    return kv, qkv


def _concat(kv, qkv, P, which):
    B = qkv.shape[0]
    return torch.cat([kv[:, :P, which - 1].expand(B, -1, -1, -1), qkv[:, :, which]], dim=1).contiguous()


@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("Tq", [129, 200, 257, 321])
@pytest.mark.parametrize("P", [64, 256, 320])
@pytest.mark.parametrize("B,H", [(1, 2), (3, 2), (1, 8)])
def test_prefix_attention_is_the_shipped_entry_on_concatenated_keys(ops, B, H, P, Tq, pre):
    kv, qkv = _inputs(ops, B, H, P, Tq, pre)
    q, k, v = qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2]            # thirds of a packed qkv
    k_pre, v_pre = kv[0, :P, 0], kv[0, :P, 1]                     # strided views of a [1, cap, 2, H, 128] buffer
    want = ops.attention(q, _concat(kv, qkv, P, 1), _concat(kv, qkv, P, 2), P, prescaled=pre)
    got = ops.attention_prefix(q, k, v, k_pre, v_pre, prescaled=pre)
    assert got.shape == want.shape == (B, Tq, H, 128)
    assert torch.equal(got.view(torch.int16), want.view(torch.int16))
    # the plane of a LONGER prefix serves a shorter one (one plane per reference and layer, every checkpoint reads its first columns)
    kv2 = poisoned((1, P + 128 + SLACK, 2, H, 128), BF)
    kv2[:, :P] = kv[:, :P]
    kv2[:, P:P + 128] = rnd((1, 128, 2, H, 128), gen(5))
    plane = ops.attention_prefix_vt(kv2[0, :P + 128, 1])
    assert plane.shape == (H, 128, P + 128)
    got2 = ops.attention_prefix(q, k, v, kv2[0, :P, 0], None, vt_pre=plane, prescaled=pre)
    assert torch.equal(got2.view(torch.int16), want.view(torch.int16))


@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("P", [64, 256, 320])
def test_prefix_attention_vs_fp64(ops, P, pre):
    B, H, Tq = 3, 2, 321
    kv, qkv = _inputs(ops, B, H, P, Tq, pre)
    got = ops.attention_prefix(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], kv[0, :P, 0], kv[0, :P, 1], prescaled=pre).double()
    kc, vc = _concat(kv, qkv, P, 1), _concat(kv, qkv, P, 2)
    rows = P + torch.arange(Tq, device=DEV)
    c = ops.attn_q_scale(128)
    worst_rl2 = worst_abs = 0.0
    for b in range(B):
        q = qkv[b, :, 0].double() / c if pre else qkv[b, :, 0]
        ref = causal_attention64(q, kc[b], vc[b], rows)
        worst_rl2 = max(worst_rl2, max(((got[b, :, h] - ref[:, h]).norm() / ref[:, h].norm()).item() for h in range(H)))
        worst_abs = max(worst_abs, ((got[b] - ref).abs() - ref.abs() * 2 ** -7).max().item())
    print(f"[attention_prefix P={P} Tq={Tq}{' pre-scaled q' if pre else ''}] worst head rel-L2 {worst_rl2:.3e}, worst |err| - 2^-7|ref| = {worst_abs:.3e}")
    assert worst_rl2 < 4e-3
    assert worst_abs < 2e-2


def test_refusals_before_any_launch(ops):
    one = ctypes.c_void_p(16)                                      # non-null, aligned, never dereferenced

    def call(P, Tq, row=None):
        row = max(P, 64) if row is None else row
        return ops.lib.evo_attn_fwd_prefix_bf16(one, one, one, one, one, one, 1, 2, Tq, P, 768 * Tq, 768, 128, 768 * Tq, 768, 128, 768 * Tq, 768, 128,
                                                512, 128, row, 1.0, one, None)
    assert call(0, 200) == -1 and call(96, 200) == -1 and call(64, 128) == -1
    assert call(128, 200, row=64) == -1                            # plane narrower than the prefix
    assert ops.lib.evo_attn_prefix_vt_bf16(one, one, 100, 2, 512, 128, 64, None) == -1
    qkv = torch.zeros(1, 200, 3, 2, 128, dtype=BF, device=DEV)
    kv = torch.zeros(1, 256, 2, 2, 128, dtype=BF, device=DEV)
    for P, T in ((0, 200), (96, 200), (64, 128)):
        with pytest.raises(RuntimeError):
            ops.attention_prefix(qkv[:, :T, 0], qkv[:, :T, 1], qkv[:, :T, 2], kv[0, :P, 0], kv[0, :P, 1])


# ------------------------------------------------------------------------------------------------ arena
@covers("evo_attn_fwd_prefix_bf16", "evo_attn_prefix_vt_bf16")
@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("B,H,P,Tq", [(2, 2, 64, 129), (1, 2, 256, 200), (3, 1, 320, 321), (1, 8, 128, 257)])
def test_arena_prefix_attention(B, H, P, Tq, pre):
    """q / k / v thirds of a packed qkv, the prefix a view of a KV cache whose rows behind P hold 0xFF; the prefix plane, the suffix
    planes and the output are allocated by the binding (carved)."""
    from evo_amd.ops import default_ops
    ops, g = default_ops(), gen(P + Tq)
    kv = poisoned((1, P + SLACK, 2, H, 128), BF)
    kv[:, :P] = rnd((1, P, 2, H, 128), g)
    inp = {"qkv": rnd((B, Tq, 3, H, 128), g, ops.attn_q_scale(128) if pre else 1.0), "kv": kv}
    _run(lambda qkv, kv: ops.attention_prefix(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], kv[0, :P, 0], kv[0, :P, 1], prescaled=pre), inp,
         expect=["evo_attn_fwd_prefix_bf16", "evo_attn_prefix_vt_bf16"])


@covers("evo_attn_prefix_vt_bf16")
@pytest.mark.parametrize("H,P,cols", [(2, 1, 64), (2, 100, 128), (3, 700, 1024)])
def test_arena_prefix_plane(H, P, cols):
    """Ragged key counts; a plane wider than its keys: the columns behind the last written tile stay poison."""
    from evo_amd.ops import default_ops
    ops = default_ops()
    kv = poisoned((1, P + SLACK, 2, H, 128), BF)
    kv[:, :P] = rnd((1, P, 2, H, 128), gen(P))
    _run(lambda kv: ops.attention_prefix_vt(kv[0, :P, 1], cols)[:, :, :(P + 63) // 64 * 64], {"kv": kv}, expect=["evo_attn_prefix_vt_bf16"])
