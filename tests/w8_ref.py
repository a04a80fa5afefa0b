"""TEST INFRASTRUCTURE (never imported by the product) for the opt-in FP8 (e4m3fn) decode weights:

  * `W8OracleOps`: the fp64 oracle backend + the optional group "w_fp8" -- every FP8 method dequantises the record and calls the
    parent's method, so a model on it computes exactly what the same model computes on the dequantised weights;
  * the SECOND exact design, `make_w4`: integers in [-15, 15] -- four significant bits, all of e4m3fn's -- times a per-row 2^g.  It uses
    the format (tests/dense_exact.py's weights need two bits) and keeps every fp32 partial sum exact (tests/test_w8_host.py proves the
    bound for every K below);
  * the shape tables tests/test_gpu_w8.py runs, kept here so that the CPU module checks the bound at every K the GPU module uses.
"""
import torch

import dense_exact as DX
from evo_amd.sh.cache import Fp8Weight, fp8_row_rule
from test_ragged_prefill_host import RaggedOracleOps


class W8OracleOps(RaggedOracleOps):
    """+ the optional group "w_fp8": dequantise, then the parent's method."""

    def __init__(self, act=torch.float64):
        super().__init__(act)
        self.w8_calls = {"quant": 0, "linear": 0, "norm_linear": 0, "hyena": 0, "gate": 0}

    def _w(self, rec):
        return rec.dequantize(torch.float64)

    def w_quant_fp8(self, w):
        self.w8_calls["quant"] += 1
        return Fp8Weight(*fp8_row_rule(w))

    def linear_w8(self, x, rec, b=None):
        self.w8_calls["linear"] += 1
        return self.linear(x, self._w(rec), b)

    def linear_residual_w8_(self, res, x, rec, bias=None):
        self.w8_calls["linear"] += 1
        return self.linear_residual_(res, x, self._w(rec), bias=bias)

    def norm_linear_w8(self, x, scale, eps, rec, b=None):
        self.w8_calls["norm_linear"] += 1
        return self.norm_linear(x, scale, eps, self._w(rec), b)

    def hyena_decode_fused_w8(self, x, norm_scale, eps, rec, proj_b, fir_state, iir_state, fir_w, fir_b, poles, residues, dskip, n_heads):
        self.w8_calls["hyena"] += 1
        return self.hyena_decode_fused(x, norm_scale, eps, self._w(rec), proj_b, fir_state, iir_state, fir_w, fir_b, poles, residues, dskip,
                                       n_heads)

    def mlp_gate_w8(self, x, rec, norm_scale=None, eps=0.0, grouped=False):
        self.w8_calls["gate"] += 1
        w = self._w(rec)
        if grouped:                                          # blocks of [32 rows of W1 | the same 32 of W2] -> [W1; W2]
            w = w.view(-1, 2, 32, w.shape[1]).transpose(0, 1).reshape(w.shape)
        return self.mlp_gate(x, w, norm_scale, eps)


# ---- the second exact design ----------------------------------------------------------------------------------------------------------------
# Bound (proved per K in tests/test_w8_host.py).  x: multiples of 1/u in [-4, 4] (u = 1 or 16, dense_exact.make_x); bytes: integers
# in [-15, 15].  The kernel sums x . bytes first: multiples of 1/u, |sum| <= 60 K, i.e. 60 K u <= 10,567,680 units at K = 11,008, u = 16
# -- below 2^24, exact in any order.  The row's 2^g then rescales (exact: it moves the exponent, not the bit count).  With bias (quarters,
# |b| <= 8) and residual (quarters, |r| < 64) the final sum is a multiple of min(2^g / u, 1/4) of magnitude <= 60 K 2^g + 72: for g in
# W4_G = [-4, 2] that is at most (60 K 2^g + 72) / min(2^g / 16, 1/4) < 2^24 units at every K below (g = 2: 4 (60 K 4 + 72); g = -4:
# 60 K 16 + 72 * 256).  g's range did not have to shrink for any shape.
W4_G = (-4, 2)


def make_w4(N, K, seed=11, device="cpu", g=W4_G):
    """[N, K] bf16: integers in [-15, 15] times 2^g_n, g_n hashed per row from g[0] .. g[1]."""
    ge = DX.ints(N, 1, g[0], g[1], 12000 + seed, device)[:, 0]
    w = DX.ints(N, K, -15, 15, 11000 + seed, device) * torch.ldexp(torch.ones(N, dtype=torch.float64, device=device), ge.to(torch.int32))[:, None]
    return w.to(torch.bfloat16)


def make_gate_w4(I, K, seed=13, device="cpu"):
    """[W1; W2] of the second design: W1 = integers in [-15, 15] times 2^-10 (at K = 4,096 u = z1 has a standard deviation of ~1.5: inside
    the GELU's curved range), W2 = integers in [-15, 15] times 2^-3."""
    w = DX.ints(2 * I, K, -15, 15, 13000 + seed, device)
    w[:I] *= 2.0 ** -10
    w[I:] *= 2.0 ** -3
    return w.to(torch.bfloat16)


DESIGNS = {"dense_exact": (DX.make_w, DX.make_gate_weights), "fourbit": (make_w4, make_gate_w4)}

# ---- the shapes tests/test_gpu_w8.py runs (N, K), every M in 1 .. 8.  At 16 weights per lane a wave's slice is 1,024 k wide:
#   K = 16      one weight vector: 63 lanes without work            K = 272     a partly filled slice (17 vectors)
#   K = 1,024   exactly one slice                                   K = 2,064   one paired trip plus a partial slice (129 vectors)
#   K = 4,096   two paired trips (unsplit); one slice per wave (SPLIT)          K = 11,008  688 vectors: SPLIT waves 0-2 take three slices, wave 3 two
# N: 37, 4,095, 8,200 are no multiples of the 4 rows per wave.  SPLIT (N <= 4,096 and K >= 2,048): the narrow layers.
PLAIN = [(37, 16), (37, 272), (8200, 1024), (4095, 2064), (37, 2064), (4096, 4096), (8200, 4096), (4096, 11008), (37, 11008)]
PLAIN_SPLIT = {(N, K): N <= 4096 and K >= 2048 for N, K in PLAIN}
GATE = [(40, 16), (40, 272), (64, 1024), (40, 2064), (1408, 4096), (64, 11008)]          # (I, K), without the norm: every M in 1 .. 8
# the norm-folding forms on dense_exact.make_norm_rows (K a power of four): K = 4,096 is the LDS-staged form (M 1 .. 8), 256 and 1,024 the
# unstaged one (M 1 .. 4; 16 vectors: a partly filled slice; 64: exactly one)
NORM_LINEAR = [(4104, 4096), (12288, 4096), (4104, 256), (4104, 1024)]
NORM_GATE = [(1408, 4096), (64, 256), (64, 1024)]
HYENA = [(4096, (1, 4, 5, 8)), (256, (1, 2, 3, 4)), (1024, (1, 2, 3, 4))]                 # (D, the M whose outputs are judged)
QUANT = [(N, K) for N in (1, 37, 4096) for K in (16, 272, 4096, 11008)]


def all_reductions():
    return sorted({k for _, k in PLAIN + GATE + NORM_LINEAR + NORM_GATE} | {d for d, _ in HYENA})


def quant_rows(N, K, seed=0):
    """[N, K] bf16 for the quantiser: random rows over many octaves, an all-zero row, a row whose maximum is its last element, rows whose
    maximum sits on either side of 448 2^e (1.75 and its bf16 neighbours), a subnormal row (the clamp at -126) and a huge one."""
    g = torch.Generator().manual_seed(1000 * N + K + seed)
    w = torch.randn(N, K, generator=g) * torch.exp2(torch.randint(-20, 20, (N, 1), generator=g).float())
    w = w.bfloat16()
    special = []
    z = torch.zeros(K)
    special.append(z.clone())
    last = torch.full((K,), 0.01)
    last[-1] = 5.0
    special.append(last)
    for top in (1.75, 1.7578125, 1.7421875, 448.0, 450.0, 446.0):       # 448 = 1.75 * 2^8; its neighbours in bf16 on both sides
        r = torch.full((K,), 0.3)
        r[K // 2] = -top
        special.append(r)
    special.append(torch.full((K,), 2.0 ** -130))                          # below the clamp: e = -126
    special.append(torch.full((K,), 2.0 ** 127))                           # e = 119
    special.append(torch.full((K,), 3.0e38))                               # beyond 448 2^119: e = 120 (the upper clamp's neighbourhood)
    for i, r in enumerate(special[:N]):
        w[(i * 7) % N] = r.bfloat16()
    return w
