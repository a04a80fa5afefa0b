"""TEST INFRASTRUCTURE (never imported by the product): input constructors and fp64 references for the ROW-LOCAL kernels -- the fused
scoring tail (csrc/score_tail.hip, evo_logprob_entropy), the GELU gate, RMSNorm / its factor kernel and the rotary kernel
(csrc/elementwise.hip) -- in the style of tests/gpu_ref64.py.  Everything here is eager torch on whatever device the inputs live on; no
kernel of libevo_mi355x.so is called.  tests/test_rowlocal_host.py pins the constructors' invariants and these references to
oracle/stripedhyena_ref.py (1e-12) on the CPU; tests/test_gpu_rowlocal.py uses them as the yardstick.

Every bound below is PER ELEMENT and has no tensor-wide `max` term: one rounding of the output format plus the fp32 arithmetic the
kernel is documented to do, each term named where it is added.
"""
import math

import torch

V = 512                       # vocabulary of the scoring tail (4 waves x 128 columns)
ROWS = 64                     # rows of one workgroup of the scoring tail: two 32-row halves
TIE_COLS = (0, 128, 256, 384)  # one column per wave: the planted row maximum is tied across them
ANTI_T, ANTI_C = 266, 267     # emb[ANTI_C] = -emb[ANTI_T]: the planted row has +32 on ANTI_C and -32 on its target ANTI_T
BF16_TINY = 2.0 ** -133       # the smallest bf16 subnormal
BF16_MAX = (2.0 - 2.0 ** -7) * 2.0 ** 127


# =========================================================================================== 1. scoring tail on exact logits
def half_index(m):
    """(k, half) of row m: the row's 32-row half inside its 64-row workgroup and its running index k among the rows of that half."""
    return (m // ROWS) * 32 + m % 32, (m % ROWS) // 32


def exact_targets(M):
    """Row m -> target (129 k) mod 512 with k = half_index(m): 129 is odd, so 512 consecutive k of one half visit every column once,
    and k = 0 .. 7 visit every (wave = n >> 7, lane half = (n >> 2) & 1) pair: 0, 129, 258, 387, 4, 133, 262, 391."""
    m = torch.arange(M)
    k = (m // ROWS) * 32 + m % 32
    return (k * 129) % V


def target_coverage(target):
    """[2, 512] counts: how often column n is the target of a row in half h of a workgroup (out-of-range targets are not counted)."""
    M = target.numel()
    m = torch.arange(M)
    half = (m % ROWS) // 32
    cov = torch.zeros(2, V, dtype=torch.int64)
    ok = (target >= 0) & (target < V)
    cov.index_put_((half[ok], target[ok].long()), torch.ones(int(ok.sum()), dtype=torch.int64), accumulate=True)
    return cov


# the planted rows, by the row's index k inside its half (both halves get them: rows k and 32 + k of the first workgroup)
PLANTS = {0: "dominant", 1: "dominant", 2: "dominant", 3: "dominant", 4: "dominant", 5: "dominant", 6: "dominant", 7: "dominant",
          8: "flat", 9: "tie", 10: "anti"}


def exact_logit_case(M, K, seed=0):
    """hidden [M, K] bf16, emb [512, K] bf16, target [M] int64 and the planted rows {row: kind} such that EVERY logit hidden @ emb^T is an
    integer multiple of 1/8 with |logit| <= 32: exact in fp32 under any summation order and exact in bf16.

    hidden: integers in [-4, 4].  emb: each row has exactly nnz = min(64, K) nonzeros, each +-2^-3 * (64 / nnz) (K = 32 cannot hold 64
    nonzeros: 32 of +-2^-2), so |logit| <= nnz * 4 * 2^-3 * 64 / nnz = 32.  Designed columns: TIE_COLS have pairwise disjoint supports
    (K >= 256) or identical rows (K < 256); emb[ANTI_C] = -emb[ANTI_T].  target = exact_targets(M); the rows with k < 11 (half_index)
    are planted (PLANTS), overriding the random hidden row:
      dominant  +4 sign(emb[t]) on the support of the row's own target t: logit[t] = 32, log-prob ~ 0, entropy ~ 0; over k = 0 .. 7 the
                row maximum sits in every wave and every lane half
      flat      hidden = 0: every logit 0, log-prob -log 512, entropy log 512
      tie       +4 sign on the supports of TIE_COLS: the row maximum 32 is tied across the four waves
      anti      +4 sign(emb[ANTI_C]) on its support: logit[ANTI_C] = 32 and the target ANTI_T (= 129 * 10 mod 512) at -32: log-prob ~ -64
    """
    g = torch.Generator().manual_seed(1000 * seed + 7 * K + M)
    nnz = min(64, K)
    val = 2.0 ** -3 * (64 // nnz)
    emb = torch.zeros(V, K, dtype=torch.float64)
    for n in range(V):
        sup = torch.randperm(K, generator=g)[:nnz]
        emb[n, sup] = val * (torch.randint(0, 2, (nnz,), generator=g).double() * 2 - 1)
    if K >= 256:
        for i, n in enumerate(TIE_COLS):
            emb[n] = 0
            emb[n, 64 * i:64 * i + 64] = val * (torch.randint(0, 2, (64,), generator=g).double() * 2 - 1)
    else:
        for n in TIE_COLS[1:]:
            emb[n] = emb[TIE_COLS[0]]
    emb[ANTI_C] = -emb[ANTI_T]
    hidden = torch.randint(-4, 5, (M, K), generator=g).double()
    target = exact_targets(M)
    plants = {}
    for m in range(min(M, ROWS)):
        k, _ = half_index(m)
        kind = PLANTS.get(k)
        if kind is None:
            continue
        plants[m] = kind
        if kind == "dominant":
            hidden[m] = 4 * torch.sign(emb[target[m]])
        elif kind == "flat":
            hidden[m] = 0
        elif kind == "tie":
            hidden[m] = 0
            for n in (TIE_COLS if K >= 256 else TIE_COLS[:1]):
                hidden[m] += 4 * torch.sign(emb[n])
        elif kind == "anti":
            assert int(target[m]) == ANTI_T
            hidden[m] = 4 * torch.sign(emb[ANTI_C])
    return dict(hidden=hidden.to(torch.bfloat16), emb=emb.to(torch.bfloat16), target=target, plants=plants)


def logits64(hidden, emb):
    return hidden.double() @ emb.double().t()


def logprob_entropy64(logits, target=None, sel=None):
    """fp64 log_softmax of the logits, per row: (log-prob of the target -- 0 where the target is outside [0, V) --, entropy,
    log-probs of the columns `sel` [M, len(sel)])."""
    lsm = torch.log_softmax(logits.double(), dim=-1)
    ent = -(lsm.exp() * lsm).sum(-1)
    lp = None
    if target is not None:
        tg = target.to(lsm.device)
        ok = (tg >= 0) & (tg < lsm.shape[-1])
        lp = lsm.gather(-1, torch.where(ok, tg, torch.zeros_like(tg)).long().unsqueeze(-1)).squeeze(-1)
        lp = torch.where(ok, lp, torch.zeros_like(lp))
    sl = lsm[:, list(sel)] if sel is not None else None
    return lp, ent, sl


def logprob_entropy_f32(logits, target=None, sel=None):
    """The kernels' FORMULA in eager fp32 torch on the same logits: x - max - log sum exp(x - max); entropy log S - sum e d / S with
    d = x - max, e = exp d.  Its error against logprob_entropy64 is the yardstick the kernels' error is measured by."""
    x = logits.float()
    mx = x.amax(-1, keepdim=True)
    d = x - mx
    e = torch.exp(d)
    s = e.sum(-1, keepdim=True)
    logz = torch.log(s)
    lsm = d - logz
    ent = (logz - (e * d).sum(-1, keepdim=True) / s).squeeze(-1)
    lp = None
    if target is not None:
        tg = target.to(x.device)
        ok = (tg >= 0) & (tg < x.shape[-1])
        lp = lsm.gather(-1, torch.where(ok, tg, torch.zeros_like(tg)).long().unsqueeze(-1)).squeeze(-1)
        lp = torch.where(ok, lp, torch.zeros_like(lp))
    sl = lsm[:, list(sel)] if sel is not None else None
    return lp, ent, sl


def measured_allowance(ref, f32):
    """Per-row allowance for a kernel's error against the fp64 value `ref`: 4 x the largest error of the fp32 restatement `f32` of the
    same formula on the same logits (the convention of tests/test_gpu_sample.py), with a floor of 2^-22 (1 + |ref|) for rows where
    the restatement happens to be exact.  Returns (allowance tensor, the restatement's largest error)."""
    e32 = float((f32.double() - ref).abs().max())
    return torch.clamp(2.0 ** -22 * (1 + ref.abs()), min=4 * e32), e32


# =========================================================================================== 2. GELU gate
def all_finite_bf16():
    """All 65,280 finite bf16 bit patterns (incl. +-0 and the subnormals) as a bf16 vector, in bit-pattern order."""
    bits = torch.arange(65536, dtype=torch.int32)
    bits = bits[(bits & 0x7f80) != 0x7f80]
    return bits.to(torch.int16).view(torch.bfloat16)


def gelu_inputs(I, gate, M=None, seed=0):
    """g [M, 2 I] bf16: the u half holds every finite bf16 pattern (wrapping around; M defaults to the fewest rows that hold them all),
    the gate half a constant or, for gate = "randn", seeded normal values."""
    u = all_finite_bf16()
    if M is None:
        M = (u.numel() + I - 1) // I
    idx = torch.arange(M * I) % u.numel()
    uu = u[idx].view(M, I)
    if gate == "randn":
        ww = torch.randn(M, I, generator=torch.Generator().manual_seed(seed)).to(torch.bfloat16)
    else:
        ww = torch.full((M, I), float(gate), dtype=torch.bfloat16)
        assert float(ww[0, 0]) == float(gate)                # the constant gates are exact in bf16
    return torch.cat([uu, ww], dim=1).contiguous()


def gelu_gate64(g):
    """fp64 0.5 u (1 + erf(u / sqrt 2)) w of g = [u | w], with 1 + erf(x) evaluated as erfc(-x): no cancellation in the negative tail."""
    I = g.shape[-1] // 2
    u, w = g[..., :I].double(), g[..., I:].double()
    return 0.5 * u * torch.special.erfc(-u / math.sqrt(2.0)) * w


ERF_ERR = 4.2e-7              # csrc/common.h: the documented |error| of erf2's rational approximation


def gelu_gate_bound(g, ref):
    """2^-8 |ref| (one bf16 rounding of the output) + 0.5 |u| |w| (4.2e-7 + 2^-22) (the approximation's documented error and the fp32
    arithmetic, carried through the product) + 2^-134 (one bf16 rounding where the output is a bf16 SUBNORMAL: half the smallest one --
    2^-8 |ref| is the rounding of a normal number only, and e.g. u = 2^-133, w = 1 has the exact value 2^-134, which no bf16 holds)."""
    I = g.shape[-1] // 2
    u, w = g[..., :I].double(), g[..., I:].double()
    return 2.0 ** -8 * ref.abs() + 0.5 * u.abs() * w.abs() * (ERF_ERR + 2.0 ** -22) + 2.0 ** -134


def gelu_gate_check(got, g, ref=None):
    """(worst err / bound, flat index of the worst element, mask of the elements outside the bound) of a kernel output `got` [M, I].
    Where the exact value is beyond the bf16 range (|ref| > BF16_MAX: u ~ 3e38 times w = 30) the output must be the infinity of the
    right sign or inside the bound; a non-finite u is not judged (the caller checks its neighbours)."""
    ref = gelu_gate64(g) if ref is None else ref
    I = g.shape[-1] // 2
    u = g[..., :I].double()
    gd = got.double()
    err = (gd - ref).abs()
    bound = gelu_gate_bound(g, ref)
    over = (ref.abs() > BF16_MAX) & torch.isinf(gd) & (torch.sign(gd) == torch.sign(ref))
    err = torch.where(over, torch.zeros_like(err), err)
    judged = torch.isfinite(u)
    ratio = torch.where(judged, err / bound, torch.zeros_like(err))
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    worst = int(ratio.argmax())
    return float(ratio.reshape(-1)[worst]), worst, ratio > 1


# =========================================================================================== 3. RMSNorm
RMS_REGIMES = ("randn", "big", "small", "outlier", "zero_row", "subnormal_row")


def rmsnorm_inputs(M, D, regime, seed=0):
    """x [M, D] bf16 and scale [D] bf16 (1 + 0.1 randn).  randn; big / small: randn x 2^+-40; outlier: channel D // 3 at 10^4 x the rest;
    zero_row: row M // 2 is zero; subnormal_row: row M // 2 holds bf16 subnormals (k 2^-133, k in [-127, 127])."""
    g = torch.Generator().manual_seed(100 * seed + D + M % 97)
    x = torch.randn(M, D, generator=g).double()
    if regime == "big":
        x = x * 2.0 ** 40
    elif regime == "small":
        x = x * 2.0 ** -40
    elif regime == "outlier":
        x[:, D // 3] = x[:, D // 3] * 1e4
    elif regime == "zero_row":
        x[M // 2] = 0
    elif regime == "subnormal_row":
        x[M // 2] = torch.randint(-127, 128, (D,), generator=g).double() * BF16_TINY
    else:
        assert regime == "randn", regime
    scale = (1 + 0.1 * torch.randn(D, generator=g)).to(torch.bfloat16)
    return x.to(torch.bfloat16), scale


def rmsnorm64(x, scale, eps, bias=None):
    """(updated row as the kernel stores it = bf16(x + bias), fp64 norm of that row): tests/gpu_ref64.rmsnorm64 on the updated rows."""
    from gpu_ref64 import rmsnorm64 as _rms
    xn = x if bias is None else (x.double() + bias.double()).to(torch.bfloat16)     # (the sum of two bf16 is exact in fp64: ONE rounding)
    return xn, _rms(xn.double(), scale, eps)


def rstd64(x, eps):
    """fp64 1 / (rms(row) + eps), eps outside the root."""
    xd = x.double()
    return 1.0 / (torch.linalg.vector_norm(xd, dim=-1) * xd.shape[-1] ** -0.5 + eps)


def rmsnorm_bound(ref):
    """2^-8 |ref| (one output rounding) + 2^-21 |ref| (fp32 arithmetic) + 2^-133 (the smallest bf16 subnormal)."""
    return (2.0 ** -8 + 2.0 ** -21) * ref.abs() + BF16_TINY


# =========================================================================================== 4. rotary
def rope_table(T, hd, scaling=1.0, base=10000.0):
    """The model's table (oracle rotary_table): fp32 angles, cos / sin rounded to bf16 values, kept in fp32.  [T, hd / 2] each."""
    inv = 1.0 / (base ** (torch.arange(0, hd, 2, dtype=torch.float32) / hd))
    t = torch.arange(T, dtype=torch.float32) / scaling
    fr = torch.outer(t, inv)
    return torch.cos(fr).bfloat16().float(), torch.sin(fr).bfloat16().float()


def rope_table_pm1(T, hd, seed=0):
    """A table of quarter turns: (cos, sin) in {(1, 0), (0, 1), (-1, 0), (0, -1)} per (position, pair), seeded -- with a power-of-two
    q_scale the rotary kernel's output is then an exact signed permutation of its input."""
    q = torch.randint(0, 4, (T, hd // 2), generator=torch.Generator().manual_seed(seed + T + hd))
    cos = torch.tensor([1.0, 0.0, -1.0, 0.0])[q]
    sin = torch.tensor([0.0, 1.0, 0.0, -1.0])[q]
    return cos.contiguous(), sin.contiguous()


def rope64(qkv, cos, sin, q_scale=1.0):
    """fp64 NeoX rotary (pairs i, i + hd / 2) of the q and k thirds of qkv [B, T, 3, H, hd] with the table cos / sin [T, hd / 2]; the q
    third times float32(q_scale) (the factor as the C ABI receives it); v untouched.  Returns (out, |x0| + |x1| per output element)."""
    x = qkv.double()
    hd = x.shape[-1]
    c = cos.double()[None, :, None, None, :]
    s = sin.double()[None, :, None, None, :]
    x0, x1 = x[:, :, :2, :, :hd // 2], x[:, :, :2, :, hd // 2:]
    rot = torch.cat([x0 * c - x1 * s, x0 * s + x1 * c], dim=-1)
    qs = float(torch.tensor(q_scale, dtype=torch.float32))
    out = x.clone()
    out[:, :, 0] = rot[:, :, 0] * qs
    out[:, :, 1] = rot[:, :, 1]
    mag = torch.zeros_like(x)
    mag[:, :, :2] = torch.cat([x0.abs() + x1.abs()] * 2, dim=-1)
    return out, mag


def rope_bound(ref, mag):
    """2^-8 |ref| (one output rounding) + 2^-23 (|x0| + |x1|) (the fp32 sum of two exact products, then the factor)."""
    return 2.0 ** -8 * ref.abs() + 2.0 ** -23 * mag
