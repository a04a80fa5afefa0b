"""TEST INFRASTRUCTURE (never imported by the product): EXACT inputs for the fused single-token Hyena launches
(evo_hyena_decode_fused_small_m, evo_hyena_decode_fused_small_m_w8: pre-norm -> projection + bias -> FIR step -> modal step -> gate, both
carried states updated in place).  New members of the two families of tests/hyena_exact.py, made so that the launch's OWN norm and
projection produce the family's z exactly; `hyena_exact.reference(..., check=<family>)` decides whether they qualify.  Eager torch on
whatever device is asked for; no kernel is called.  tests/test_hyena_fused_exact_host.py pins the design on the CPU,
tests/test_gpu_hyena_fused_exact.py uses it (PARITY row 9e).

The construction, for a token row x of width D in {256, 1024, 4096} (sqrt(D) a power of two):
  norm        source integers s[k] in [-2, 2] in the first D - 4 columns, x[k] = 32 s[k]; the last four columns hold ballast x = 32 q_i with
              q_0^2 + .. + q_3^2 = 4 D - sum s^2 (Lagrange; q_i <= 128).  Then sum x^2 = 4096 D in fp32 in any order (every partial sum a
              multiple of 1024 below 2^24 + 1), sqrtf = 64 sqrt(D), * (1 / sqrtf(D)) = 64, + 1e-6 = 64, inv = 2^-6, and with g = 1 the
              normalised row is s / 2 (ballast q / 2): exactly, statement by statement (dense_exact.rmsnorm_fp32_emulated).
  projection  W [3 D, D] has at most ONE non-zero per row, +-2 at a source column, none in the ballast columns; some rows are all zero.
              So z = +-s + b with one product per sum: exact in any order, integers in [-3, 3], bf16 without rounding.  max |row| is 2 or 0:
              W is a fixed point of evo_amd.sh.cache.fp8_row_rule (bytes 256 at scale 2^-7) and serves the FP8 entry unchanged.  Each
              third (x2 | x1 | v) of a head reads the sources through its own (column map, sign) pair.
  U           dense sources, bias in {-1, 0, 1}, one row in sixteen of W zero; filters as family_u; a random FIR history and start state.
  I           the x2 rows of W are zero (x2 == 1 through the FIR bias; their z is the bias, integers in [-2, 2]); x1 and v of a channel read
              the SAME source with their own signs, so x1 v = +-s^2 (1 or 4) at the one step the source is non-zero -- in the first
              `I_IMPULSE_STEPS` steps, for every second (row, source) -- and 0 otherwise.  Filters as family_i (eight distinct dyadic
              poles per channel, so the poles of neighbouring channels differ).  The start state s0: everywhere on the (row, channel)
              pairs with no impulse -- its response decays through fp32's flush region inside the run -- and only at the modes with
              |p| in {0, 1} on the pairs with one (a decaying remnant of s0 under an impulse would need more than 16 bits).

Rows are independent, so one data set at the largest M serves every smaller M as its first rows (`Fused.rows`)."""
import math
from collections import namedtuple
from functools import lru_cache

import torch

import hyena_exact as X

BF = X.BF
Fused = namedtuple("Fused", "fam xs g W b prm hist s0 z ref H")
# xs    [T, M, D] bf16: the token rows, step by step          g  [D] bf16: the norm's scale (ones)
# W     [3 D, D] bf16, b [3 D] bf16: the projection           prm  (fir_w, fir_b, poles, residues, dskip)
# hist  [M, 2, 3 D] bf16: the FIR history before step 0 (fir_state = hist.transpose(1, 2))
# s0    [M, D, 8] complex128: the modal state before step 0 (Gaussian integers)
# z     [M, T, 3 D] bf16: what norm -> projection + bias must give          ref  hyena_exact.Ref of (z, prm, hist, s0), every step's state

U_STEPS, I_STEPS, I_IMPULSE_STEPS = 40, 140, 40
# (D, every M): D = 4096 the LDS-staged form (one channel per wave); 256 / 1024 the unstaged forms (one channel per wave at M = 1, 4, two
# at M = 2, 3; 256: 32 vectors, the single-slice loop; 1024: 128 vectors, one paired trip)
SHAPES = [(4096, tuple(range(1, 9))), (256, (1, 2, 3, 4)), (1024, (1, 2, 3, 4))]
SEED = 23
# which family sees which of the single-token launches' mutants in y, the FIR history or the modal state, over the runs above -- at EVERY
# (D, M) (state_prev_row: M >= 2); asserted in tests/test_hyena_fused_exact_host.py
MUTANTS = ["state_prev_row", "chan_xor1", "fir_old_kept", "state_early"]
CAUGHT = {"state_prev_row": (True, True), "chan_xor1": (True, True), "fir_old_kept": (True, True), "state_early": (True, True)}


def steps(fam):
    return U_STEPS if fam == "U" else I_STEPS


@lru_cache(maxsize=None)
def four_squares(n):
    """(a, b, c, d), a >= b >= c >= d >= 0, with a^2 + b^2 + c^2 + d^2 = n."""
    for a in range(math.isqrt(n), -1, -1):
        r1 = n - a * a
        for b in range(min(a, math.isqrt(r1)), -1, -1):
            r2 = r1 - b * b
            for c in range(min(b, math.isqrt(r2)), -1, -1):
                if 2 * c * c < r2:
                    break
                d = math.isqrt(r2 - c * c)
                if d * d == r2 - c * c and d <= c:
                    return a, b, c, d
    raise AssertionError(n)


def token_rows(src):
    """src [..., D - 4] integers in [-2, 2] -> (xs [..., D] bf16, the normalised rows [..., D] fp64 the norm must give)."""
    D = src.shape[-1] + 4
    assert D in (256, 1024, 4096)
    rest = (4 * D - (src * src).sum(-1)).to(torch.int64)
    q = torch.tensor([four_squares(int(n)) for n in rest.reshape(-1).tolist()], dtype=torch.float64).reshape(*src.shape[:-1], 4)
    full = torch.cat([src.double(), q], -1)
    return (32.0 * full).to(BF), full / 2


def projection(g, D, H, zero_x2, same_source, zero_share):
    """-> (W [3 D, D] bf16, col [3 D] int64, sign [3 D] fp64 (0: an all-zero row)): row j = (head, third, c) reads source column col[j]."""
    hd = D // H
    j = torch.arange(3 * D)
    third, ch = (j // hd) % 3, (j // (3 * hd)) * hd + j % hd
    maps = [torch.randperm(D, generator=g) % (D - 4) for _ in range(3)]
    if same_source:
        maps[2] = maps[1]
    col = torch.stack(maps)[third, ch]
    sign = 2.0 * X._ri(g, 0, 1, (3 * D,)) - 1
    if zero_share:
        sign = sign * (torch.rand(3 * D, generator=g) >= zero_share).double()
    if zero_x2:
        sign = sign * (third != 0).double()
    W = torch.zeros(3 * D, D, dtype=torch.float64)
    W[j, col] = 2.0 * sign
    return W.to(BF), col, sign


def _z(norm, col, sign, b):
    """norm [T, M, D] fp64 -> z [M, T, 3 D] bf16 = norm W^T + b, by its one product per row (the host module redoes it as a matrix product)."""
    z = sign * 2.0 * norm[..., col] + b.double()
    zb = z.to(BF)
    assert torch.equal(zb.double(), z)
    return zb.transpose(0, 1).contiguous()


def fused_u(M, T, D, H, seed, device="cpu"):
    g = X._gen(seed)
    xs, norm = token_rows(X._ri(g, -2, 2, (T, M, D - 4)))
    W, col, sign = projection(g, D, H, zero_x2=False, same_source=False, zero_share=1.0 / 16)
    b = X._ri(g, -1, 1, (3 * D,)).to(BF)
    z = _z(norm, col, sign, b)
    fir_w = X._ri(g, -1, 1, (3 * D, 3)).to(BF)
    fir_b = X._ri(g, -1, 1, (3 * D,)).to(BF)
    poles = torch.tensor(X._U_POLES, dtype=torch.float32)[torch.randint(0, 4, (D, 8), generator=g)].contiguous()
    residues = (X._ri(g, -2, 2, (D, 8, 2)) / 4).float().contiguous()
    dskip = (X._ri(g, -2, 2, (D,)) / 2).to(BF)
    hist, s0 = X._halo_s0(g, M, D, True, True)
    return _finish("U", xs, W, b, (fir_w, fir_b, poles, residues, dskip), hist, s0, z, H, device)


def fused_i(M, T, D, H, seed, device="cpu"):
    g = X._gen(seed)
    hd = D // H
    has = torch.rand(M, D - 4, generator=g) < 0.5
    t0 = torch.randint(0, min(I_IMPULSE_STEPS, T), (M, D - 4), generator=g)
    amp = X._ri(g, 1, 2, (M, D - 4)) * (2 * X._ri(g, 0, 1, (M, D - 4)) - 1)
    src = torch.where(has & (torch.arange(T)[:, None, None] == t0), amp, torch.zeros(T, M, D - 4, dtype=torch.float64))
    xs, norm = token_rows(src)
    W, col, sign = projection(g, D, H, zero_x2=True, same_source=True, zero_share=0.0)
    third = (torch.arange(3 * D) // hd) % 3
    b = torch.where(third == 0, X._ri(g, -2, 2, (3 * D,)), torch.zeros(3 * D, dtype=torch.float64)).to(BF)
    z = _z(norm, col, sign, b)
    pick = torch.stack([torch.randperm(len(X._I_POLES), generator=g)[:8] for _ in range(D)])
    poles = torch.tensor(X._I_POLES, dtype=torch.float32)[pick].contiguous()
    residues = torch.zeros(D, 8, 2)
    residues[torch.arange(D), torch.randint(0, 8, (D,), generator=g)] = \
        torch.tensor(X._I_RES, dtype=torch.float32)[torch.randint(0, len(X._I_RES), (D,), generator=g)]
    dskip = (torch.arange(D) % 2).to(BF)
    fir_w = torch.zeros(3 * D, 3)
    fir_w[third != 0, 2] = 1.0
    fir_b = (third == 0).float()
    hist, s0 = X._halo_s0(g, M, D, True, True)
    x1_rows = torch.arange(3 * D).view(H, 3, hd)[:, 1].reshape(D)                   # channel -> its x1 row of W
    impulse = has[:, col[x1_rows]]                                                  # [M, D]: this (row, channel) sees an impulse
    mag2 = poles[..., 0] ** 2 + poles[..., 1] ** 2                                  # 0, 0.25, 0.5 or 1
    keep = ~impulse[:, :, None] | ((mag2 == 0) | (mag2 == 1))[None]
    s0 = torch.where(keep, s0, torch.zeros_like(s0))
    return _finish("I", xs, W, b, (fir_w.to(BF), fir_b.to(BF), poles, residues.contiguous(), dskip), hist, s0, z, H, device)


def _finish(fam, xs, W, b, prm, hist, s0, z, H, device):
    d = lambda t: t.to(device)
    z, prm, hist, s0 = d(z), tuple(d(t) for t in prm), d(hist), d(s0)
    ref = X.reference(z, prm, H, z_halo=hist, s0=s0, check=fam)
    return Fused(fam, d(xs), torch.ones(xs.shape[-1], dtype=BF, device=device), d(W), d(b), prm, hist, s0, z, ref, H)


FAMILIES = {"U": fused_u, "I": fused_i}


def make(fam, D, M=None, device="cpu", seed=SEED):
    """The data set of (family, D) the GPU module walks: `steps(fam)` steps at the largest M of SHAPES (or M)."""
    M = max(dict(SHAPES)[D]) if M is None else M
    return FAMILIES[fam](M, steps(fam), D, D // 128, seed, device=device)


def rows(c, M):
    """The first M batch rows of a data set (rows are independent: the reference of M rows is the first M rows of the reference)."""
    return c._replace(xs=c.xs[:, :M].contiguous(), hist=c.hist[:M], s0=c.s0[:M], z=c.z[:M], ref=X.Ref(*(t[:M] for t in c.ref)))


def rounded_share(y):
    """(share of y that needs a non-trivial bf16 rounding, number of exact ties) for fp64 y that fp32 holds exactly."""
    f = y.float()
    assert torch.equal(f.double(), y)
    i = f.contiguous().view(torch.int32)
    low = i & 0xFFFF
    return float((low != 0).double().mean()), int((low == 0x8000).sum())
