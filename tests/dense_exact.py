"""TEST INFRASTRUCTURE (never imported by the product): EXACT inputs and the single-rounding reference for the dense layers
(csrc/gemm.hip, csrc/gemv.hip), in the style of tests/rowlocal_ref.py.  Everything here is eager torch on whatever device is asked for; no
kernel of libevo_mi355x.so is called.  tests/test_dense_exact_host.py pins the invariants on the CPU, tests/test_gpu_dense_exact.py uses
them as the yardstick.

The idea: with small-integer operands every fp32 partial sum of x w^T (+ bias + residual) is an integer multiple of 1/4 below 2^22 --
EXACT in fp32 in any summation order, on the VALU's dot2, on the MFMA, across LDS or a workspace.  The only rounding left is the one to
bf16 at the store, so the expected output is ONE bit pattern per element, round-to-nearest-even ties included.

  x         integers in [-4, 4]                       (the weight-streaming forms also: multiples of 1/16 in [-4, 4], see make_x)
  w         integers in [-2, 2]                       sum |x w| <= 8 K <= 88,064 < 2^24 up to K = 11,008  (K_MAX)
  bias      multiples of 1/4 in [-8, 8]
  residual  multiples of 1/4 in (-64, 64)             (at most 8 significant bits: exact in bf16)

The values are a HASH of (row, column, seed) in wrapping int64 arithmetic -- the same on every device, and the tensor of a smaller
shape is the top-left block of the larger one with the same seed: the CPU module checks blocks of the very tensors the GPU module uses.
"""
import torch

X_UNITS = (1, 16)              # make_x's two value sets: integers; multiples of 1/16
K_MAX = 11008                 # 8 K < 2^24 / ... : the widest reduction the bounds above are stated for
EPS = 1e-6                    # the model's RMSNorm eps

_MASK = (1 << 63) - 1


def _s64(v):
    """A 64-bit constant as the signed Python int torch's int64 arithmetic wants."""
    v &= (1 << 64) - 1
    return v - (1 << 64) if v >= (1 << 63) else v


_C1, _C2, _C3 = _s64(0x9E3779B97F4A7C15), _s64(0xBF58476D1CE4E5B9), _s64(0x94D049BB133111EB)


def hash31(rows, cols, seed, device="cpu"):
    """[rows, cols] int64 in [0, 2^31): a splitmix64-style mix of (row, column, seed).  int64 products wrap (two's complement) on the CPU
    and on the GPU alike, shifts are made logical by masking: the values do not depend on the device or on the shape."""
    i = torch.arange(rows, dtype=torch.int64, device=device)[:, None]
    j = torch.arange(cols, dtype=torch.int64, device=device)[None, :]
    z = i * _C1 + j * _C2 + _s64((int(seed) + 1) * _C3)
    z = (z ^ ((z >> 30) & ((1 << 34) - 1))) * _C2
    z = (z ^ ((z >> 27) & ((1 << 37) - 1))) * _C3
    z = z ^ ((z >> 31) & ((1 << 33) - 1))
    return (z >> 33) & 0x7fffffff


def ints(rows, cols, lo, hi, seed, device="cpu"):
    """Integers in [lo, hi] (float64)."""
    return (hash31(rows, cols, seed, device) % (hi - lo + 1) + lo).double()


def make_x(M, K, seed=1, device="cpu", unit=1):
    """unit = 1: integers in [-4, 4].  unit = 16 (X_UNITS, the weight-streaming forms' second data set): multiples of 1/16 in [-4, 4] --
    seven significant bits, exact in bf16; sum |x w| <= 8 K in units of 1/16 is 128 K <= 1,409,024 < 2^24, so every fp32 partial sum is
    still exact.  What it adds: a partial sum of INTEGERS below 256 is itself a bf16 number, so a partial sum that crosses LDS or the
    workspace in bf16 goes unnoticed at short reductions; a partial sum of sixteenths needs more than 8 bits from |p| >= 16 on."""
    return (ints(M, K, -4 * unit, 4 * unit, 1000 * unit + seed, device) / unit).to(torch.bfloat16)


def make_w(N, K, seed=2, device="cpu"):
    return ints(N, K, -2, 2, 2000 + seed, device).to(torch.bfloat16)


def make_bias(N, seed=3, device="cpu"):
    return (ints(1, N, -32, 32, 3000 + seed, device)[0] / 4).to(torch.bfloat16)


def make_residual(M, N, seed=4, device="cpu"):
    """Multiples of 1/4 in (-64, 64), every value of the range possible, magnitudes weighted towards the upper half (255 - u v / 256 quarter
    units, u and v uniform in 0 .. 255: mean |r| ~ 48): x w^T + b + r then needs more than bf16's 8 bits on more than 10 % of the elements
    at the SHORTEST reductions too (K = 64, where |x w^T| ~ 36: uniform magnitudes gave 9.3 %)."""
    u, v = hash31(M, N, 4000 + seed, device), hash31(M, N, 4500 + seed, device)
    mag = 255 - (u % 256) * (v % 256) // 256
    sgn = (u >> 16) % 2 * 2 - 1
    return ((mag * sgn).double() / 4).to(torch.bfloat16)


def make_gate_weights(I, K, seed=5, device="cpu"):
    """[W1; W2] ([2 I, K]) of the gated MLP: W1 = integers in [-2, 2] times 2^-7 (a power of two: the sums stay exact; at K = 4,096 u = z1 has
    a standard deviation of ~1.8, inside the GELU's curved range), W2 = integers in [-2, 2]."""
    w = ints(2 * I, K, -2, 2, 5000 + seed, device)
    w[:I] *= 2.0 ** -7
    return w.to(torch.bfloat16)


def make_pow2_rows(M, seed=6, device="cpu"):
    """A per-row factor 2^e, e in -3 .. 3, different from row to row (fp32): scaling by it is exact."""
    e = ints(M, 1, -3, 3, 6000 + seed, device)[:, 0]
    return torch.ldexp(torch.ones(M, dtype=torch.float64, device=device), e.to(torch.int32)).float()


def make_sparse_x(M, K, seed=7, device="cpu"):
    """x rows with exactly 8 nonzeros of +-1 each (the sum-of-squares producer's input: |x w^T| <= 16)."""
    h = hash31(M, K, 7000 + seed, device)
    key = h * K + torch.arange(K, dtype=torch.int64, device=device)[None, :]           # unique keys: no ties in the sort
    idx = key.argsort(dim=-1)[:, :8]
    sgn = (hash31(M, 8, 7500 + seed, device) % 2 * 2 - 1).double()
    x = torch.zeros(M, K, dtype=torch.float64, device=device)
    x.scatter_(1, idx, sgn)
    return x.to(torch.bfloat16)


def make_int_residual(M, N, seed=8, device="cpu"):
    """Integers in [-8, 8]: with make_sparse_x and make_w the stored rows are integers with |y| <= 24."""
    return ints(M, N, -8, 8, 8000 + seed, device).to(torch.bfloat16)


# ---- rows whose RMSNorm is exact -----------------------------------------------------------------------------------------------------------
NORM_EXPS = (5, 6, 8)


def make_norm_rows(M, K=4096, seed=9, device="cpu"):
    """(x [M, K] bf16, a [M] int): row m is a hashed permutation of K / 2 entries of +-1, K / 8 of +-2 and 3 K / 8 zeros, times 2^a_m with
    a_m in NORM_EXPS.  K a power of four (256, 1024, 4096), so sqrt(K) is a power of two.  Then in fp32, exactly:
      sum x^2 = (K / 2 + 4 K / 8) 4^a = K 4^a;  sqrtf = sqrt(K) 2^a;  * (1 / sqrtf(K)) = 2^a;  + 1e-6 -> 2^a (half an ulp at 32 is 1.9e-6);
      inv = 2^-a;  g x inv = integers in [-6, 6] for g in {1, 2, 3}."""
    assert K in (256, 1024, 4096)
    h = hash31(M, K, 9000 + seed, device)
    key = h * K + torch.arange(K, dtype=torch.int64, device=device)[None, :]
    rank = key.argsort(dim=-1).argsort(dim=-1)                                          # a permutation of 0 .. K - 1 per row
    mag = torch.where(rank < K // 2, 1.0, torch.where(rank < K // 2 + K // 8, 2.0, 0.0)).double()
    sgn = (hash31(M, K, 9500 + seed, device) % 2 * 2 - 1).double()
    a = torch.tensor(NORM_EXPS, device=device)[(torch.arange(M, device=device) + seed) % 3]
    x = mag * sgn * torch.ldexp(torch.ones(M, dtype=torch.float64, device=device), a.to(torch.int32))[:, None]
    return x.to(torch.bfloat16), a


def make_norm_scale(K, seed=10, device="cpu"):
    """The norm's scale g: integers in {1, 2, 3}."""
    return ints(1, K, 1, 3, 10000 + seed, device)[0].to(torch.bfloat16)


def norm_rows_expected(x, g, a):
    """What RMSNorm must return for make_norm_rows' rows, bit for bit: g x 2^-a (integers in [-6, 6])."""
    s = torch.ldexp(torch.ones(x.shape[0], dtype=torch.float64, device=x.device), (-a).to(torch.int32))
    return (g.double()[None, :] * x.double() * s[:, None]).to(torch.bfloat16)


def rmsnorm_fp32_emulated(x, g, eps=EPS):
    """The kernels' statements in numpy float32, one at a time (csrc/elementwise.hip rmsnorm_kernel: ss = sum x^2 in fp32;
    inv = 1 / (sqrtf(ss) * (1 / sqrtf(K)) + eps); out = bf16(x * inv * g))."""
    import numpy as np
    xf = x.float().numpy().astype(np.float32)
    K = xf.shape[1]
    ss = np.zeros(xf.shape[0], dtype=np.float32)
    for k in range(K):                                                                  # sequential fp32 accumulation (any order is exact here)
        ss = (ss + xf[:, k] * xf[:, k]).astype(np.float32)
    isd = np.float32(1.0) / np.sqrt(np.float32(K))
    den = (np.sqrt(ss).astype(np.float32) * isd).astype(np.float32) + np.float32(eps)
    inv = (np.float32(1.0) / den.astype(np.float32)).astype(np.float32)
    out = ((xf * inv[:, None]).astype(np.float32) * g.float().numpy()[None, :].astype(np.float32)).astype(np.float32)
    return torch.from_numpy(out), torch.from_numpy(inv)


# ---- the reference ---------------------------------------------------------------------------------------------------------------------------
def exact_product(x, w, chunk=4096):
    """S = x w^T in fp64, in row chunks (exact: integers, or multiples of 2^-7 for the gate's W1)."""
    wd = w.double().t().contiguous()
    out = torch.empty(x.shape[0], w.shape[0], dtype=torch.float64, device=x.device)
    for i in range(0, x.shape[0], chunk):
        out[i:i + chunk] = x[i:i + chunk].double() @ wd
    return out


def exact_sum(x, w, b=None, r=None, row_scale=None, S=None):
    """row_scale * S + b + r in fp64 (S = exact_product(x, w) unless given; it is not modified), asserted to equal its own fp32 cast."""
    s = exact_product(x, w) if S is None else S
    if row_scale is not None:
        s = s * row_scale.double()[:, None]
    elif b is not None or r is not None:
        s = s.clone()
    if b is not None:
        s = s + b.double()[None, :]
    if r is not None:
        s = s + r.double()
    assert torch.equal(s.float().double(), s), "the exact sum is not an fp32 number: operands outside the stated ranges"
    return s


def expected(x, w, b=None, r=None, row_scale=None, S=None):
    """bf16(row_scale * x w^T + b + r): ONE round-to-nearest-even rounding of the exact sum."""
    return exact_sum(x, w, b, r, row_scale, S).float().bfloat16()


def bits(t):
    return t.contiguous().view(torch.int16)


def mismatches(got, want):
    """Number of elements whose bf16 bit patterns differ, and the (row, column) of the first one (None when equal)."""
    assert got.shape == want.shape and got.dtype == want.dtype == torch.bfloat16, (got.shape, want.shape, got.dtype)
    ne = bits(got) != bits(want)
    n = int(ne.sum())
    return n, (tuple(ne.nonzero()[0].tolist()) if n else None)


def truncate_bf16(s):
    """bf16 by TRUNCATION of the fp32 value (what a pack without rounding would store)."""
    i = s.float().contiguous().view(torch.int32)
    return (i & -65536).view(torch.float32).bfloat16()


def shares(s):
    """(not representable in bf16, exact round-to-nearest ties, truncation gives another pattern than rounding) as fractions of the
    elements of the exact sums s (fp64 values that are fp32 numbers)."""
    f = s.float()
    i = f.contiguous().view(torch.int32)
    low = i & 0xffff
    n = s.numel()
    rne = f.bfloat16()
    return (float((low != 0).sum()) / n, float((low == 0x8000).sum()) / n, float((bits(truncate_bf16(s)) != bits(rne)).sum()) / n)


def gate_reference(S12, I):
    """g = [bf16(S1) | bf16(S2)] of the exact products S12 [M, 2 I]: what the gate kernels are documented to evaluate the GELU gate on
    (judged by rowlocal_ref.gelu_gate_check)."""
    return S12.float().bfloat16()


# ---- the shapes tests/test_gpu_dense_exact.py runs (tests/test_dense_exact_host.py checks the exactness condition for every one) -----------
PERSISTENT = [(9, 256, 64), (300, 512, 64), (513, 256, 64),                 # K = 64: the tile-per-workgroup gemm_bf16_kernel
              (256, 256, 128), (300, 512, 192), (511, 768, 4096), (2049, 4096, 4096), (257, 256, 11008),
              (8269, 4096, 128), (8448 + 44, 2048, 192)]                    # more tiles than workgroups, the ragged tile inside a workgroup's list
XBLK = [(512, 256, 128), (8448, 2048, 192)]                                 # (M, N, K), blocked-y input
GATED = [(300, 128, 128), (2049, 1408, 4096)]                               # (M, I, K)
LINEAR_T = [(2, 640, 768, 128), (3, 1026, 768, 192)]                        # (B, T, N, K): the plain and the tail form of z^T
ROW_SCALE = [(300, 512, 192), (2049, 4096, 4096)]
SUMSQ = [(M, N, 128) for M in (300, 2049 + 9, 8269) for N in (256, 4096)] + [(300, 256, 192)]
SEAM = [(4096 + 1, 512, 256), (4096 + 16, 512, 256), (4096 + 17, 512, 256)]
DOT2 = [(37, 264), (4095, 2056), (4096, 10928)]                             # (N, K), every M in 1 .. 8 (K % 32 != 0 keeps 5-8 rows on dot2)
DOT2_LE4 = [(4096, 4096), (12288, 4096), (8200, 768)]                       # M <= 4
SKINNY_M = [5, 16, 17, 32, 33, 48, 49, 64]
SKINNY_MFMA = [(37, 288), (512, 4096), (8192, 288), (8200, 288)]
SKINNY_NW = [(8200, 256), (8200, 768), (12288, 4096), (12296, 512), (16384, 256)]
SPLITK = [((33, 64), 1024, 1024, 4), ((33, 64), 1024, 2304, 8), ((33, 64), 8128, 1024, 3), ((33, 64), 4096, 512, 0),
          ((17, 32), 4096, 8192, 4), ((17, 32), 4096, 11008, 4)]            # (Ms, N, K, slices the launch must use; 0: must NOT split)
GATE_SMALL_M = [1, 2, 3, 4, 5, 6, 7, 8, 13, 17, 40, 64]
GATE_SMALL = [(40, 264), (64, 256), (1408, 4096), (11008, 4096)]            # (I, K); (40, 264): M <= 4 only
# K = 256, 1024: M <= 4, the forms that do not stage the rows in LDS (32 vectors of 8: the single-slice tail only; 128: exactly one paired trip)
NORM_LINEAR = [(4104, 4096), (12288, 4096), (4104, 256), (4104, 1024)]      # (N, K)
NORM_GATE = [(1408, 4096), (64, 256), (64, 1024)]                           # (I, K)
HYENA_FUSED = [(4096, (1, 4, 5, 8)), (256, (1, 2, 3, 4)), (1024, (1, 2, 3, 4))]   # (D, Ms)


def all_reductions():
    """Every reduction length K the GPU module uses."""
    ks = {s[2] for s in PERSISTENT + XBLK + GATED + ROW_SCALE + SUMSQ + SEAM} | {s[3] for s in LINEAR_T}
    ks |= {s[1] for s in DOT2 + DOT2_LE4 + SKINNY_MFMA + SKINNY_NW + GATE_SMALL + NORM_LINEAR + NORM_GATE} | {s[2] for s in SPLITK}
    ks |= {s[0] for s in HYENA_FUSED}
    return sorted(ks)


def through_bf16_partials(x, w, b=None, r=None, parts=8):
    """What a k-split kernel would store if its `parts` partial sums (contiguous runs of 32-k steps, as skinny_mfma_kernel's eight waves
    take them) crossed LDS in bf16: each partial rounded, then summed in fp32 with bias and residual, one more rounding."""
    K = x.shape[1]
    steps = K // 32
    acc = torch.zeros(x.shape[0], w.shape[0], dtype=torch.float32, device=x.device)
    for p in range(parts):
        k0, k1 = 32 * (steps * p // parts), 32 * (steps * (p + 1) // parts)
        if k1 > k0:
            acc = acc + (x[:, k0:k1].double() @ w[:, k0:k1].double().t()).float().bfloat16().float()
    if b is not None:
        acc = acc + b.float()[None, :]
    if r is not None:
        acc = acc + r.float()
    return acc.bfloat16()
