"""TEST INFRASTRUCTURE (never imported by the product): EXACT inputs and the per-step fp64 reference for the Hyena operator
(csrc/hyena_ct.hip, csrc/hyena.hip, csrc/hyena_ragged.hip, evo_hyena_step), as tests/dense_exact.py / tests/attn_exact.py are for the dense
layers and the attention.  Everything here is eager torch on whatever device the inputs live on; no kernel of libevo_mi355x.so is called.
tests/test_hyena_exact_host.py pins the designs on the CPU, tests/test_gpu_hyena_exact.py uses them.

The operator:  zc[t] = w0 z[t-2] + w1 z[t-1] + w2 z[t] + b  (zero where `mask` says pad);  (x2 | x1 | v) = the thirds of every head of zc;
x = x1 v;  S_t = p S_{t-1} + x_t  (8 complex modes);  y_t = (Re sum_s R_s S_t + dskip x_t) x2_t.

Two input families make every partial sum of that exactly representable in fp32 IN ANY ORDER of summation -- also through the bf16 hi + lo
operand splits of csrc/hyena_ct.hip -- so a kernel's y must be the reference rounded ONCE to bf16, and its states the reference's, bit for bit.

  U   unit poles, integer data, dense.  z integer in [-2, 2]; FIR taps and bias in {-1, 0, 1}; every pole in {1, -1, i, -i}; residues
      (integers in [-2, 2]) / 4, real and imaginary; dskip (integers in [-2, 2]) / 2.  All states are Gaussian integers, all outputs
      multiples of 1 / 8.  Asserted on the reference: |state component| < 2^16 (what a bf16 hi + lo split holds), |x1 v| < 2^8,
      8 |y| < 2^24.  A third or more of the outputs need a non-trivial bf16 rounding, many of them exact ties (round-to-nearest-EVEN).
      U cannot see a wrong POWER of a pole (p^4 = 1: p^(k + 4) = p^k and the scan constants p^(32 2^k) are all 1), hence:
  I   dyadic decaying poles, sparse impulses.  Per channel eight DISTINCT poles from {0.5 +- 0.5 i, -0.5 + 0.5 i, +-0.5, +-0.5 i, 0, 1, -i}
      and exactly one non-zero residue, from {1, i, -2, 0.5 + 0.5 i, 1 - i}, at a random mode; the FIR is the identity on x1 and v
      (tap 2 = 1), x2 == 1 through the bias; dskip = 0 in the even channels and 1 in the odd ones; x1 v != 0 only at isolated steps >= 300
      apart (first one at a random offset per (row, channel); with a start state s0 not before step 320, when s0's own response has left
      fp64's 53 bits), amplitudes +-1 .. 3.  Every output is ONE product R p^(t - t0) a -- a power of two times a small integer.  Tails
      with 0 < |ref| < 2^-100 (fp32 flushes there) are compared as |got| <= 2^-99, never skipped (`equal_or_flushed`).  Asserted: every
      state component and every y in the exact region has a significand of <= 16 bits; every channel with an impulse at least 97 steps
      before the end has one whose lags 0 .. 96 all lie in the exact region (|ref| >= 2^-100 or exactly 0; with s0 also |ref| < 2^-149,
      the remains of s0's response under an impulse response whose real part is exactly 0 -- below every fp32 number).
      evo_amd.hyena_tables.table_ok is False for these filters: that guard belongs to the model's routing (cancelling modes under white
      input); HipOps.hyena_ct does not consult it, and nothing cancels here.

The operator is causal: one reference run at the longest T serves every shorter T and every lens[b] as a prefix (`Ref.states[:, t]` is the
end state of a run of t + 1 steps -- tests/test_hyena_exact_host.py).

`mutants()`: deliberately wrong references (reference(..., mutant=name) / round_store(..., mutant=name)) -- the defects the GPU file is
there to catch; which family sees which is tabulated and asserted in tests/test_hyena_exact_host.py.  The last three are the defects of
the single-token launches (a row's modal state from the previous row, a channel's poles and residues from its pair c ^ 1, an FIR history
whose older column is never replaced); tests/hyena_fused_exact.py builds the walks that see them, tests/test_hyena_fused_exact_host.py
tabulates where."""
from collections import namedtuple

import torch

BF = torch.bfloat16
TILE, BLOCK = 512, 32                       # csrc/hyena_ct.hip: steps per tile / per block (evo_amd.hyena_tables: L = 32, NB = 16)
FLUSH, FLUSH_GOT = 2.0 ** -100, 2.0 ** -99  # family I: the tiny region and what a kernel may hold there
Ref = namedtuple("Ref", "y states hist")
# y       [B, T, D] fp64, exact
# states  [B, T, D, 8] complex128: the state after EVERY step ([B, n, D, 8] at the steps `state_at` [B, n] names)
# hist    [B, T + 2, 3 D] fp64: z behind its two history rows -- hist[:, t + 1:t + 3] is the FIR history AFTER step t

_U_POLES = [(1, 0), (-1, 0), (0, 1), (0, -1)]
_I_POLES = [(0.5, 0.5), (0.5, -0.5), (-0.5, 0.5), (0.5, 0), (-0.5, 0), (0, 0.5), (0, -0.5), (0, 0), (1, 0), (0, -1)]
_I_RES = [(1, 0), (0, 1), (-2, 0), (0.5, 0.5), (1, -1)]


def _gen(seed):
    return torch.Generator().manual_seed(int(seed))


def _ri(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def _thirds(t, H):
    """[..., 3 D] -> (x2, x1, v) [..., D]: the thirds of every head (reference column order h * 3 hd + g * hd + c)."""
    D = t.shape[-1] // 3
    t5 = t.reshape(*t.shape[:-1], H, 3, D // H)
    return tuple(t5[..., g, :].reshape(*t.shape[:-1], D) for g in range(3))


def _halo_s0(g, B, D, want_halo, want_s0):
    halo = _ri(g, -2, 2, (B, 2, 3 * D)).to(BF) if want_halo else None
    s0 = torch.complex(_ri(g, -64, 64, (B, D, 8)), _ri(g, -64, 64, (B, D, 8))) if want_s0 else None
    return halo, s0


def sig_bits_ok(x, bits):
    """x (fp64) has a significand of at most `bits` bits (0 passes)."""
    m, _ = torch.frexp(x)
    s = m * float(1 << bits)
    return s == s.round()


# ------------------------------------------------------------------------------------------------ the reference
def mutants():
    """(name, what it corrupts: "y" or "state")."""
    return [("fir_reversed", "y"),            # FIR tap order reversed
            ("tile_hist_zero", "y"),          # the FIR history of step 0 of a 512-step tile taken as zero
            ("row_hist_prev_row", "y"),       # the history of a batch row's first step taken from the previous row's last steps
            ("swap_reim", "y"),               # re / im of one mode (3) swapped in the output
            ("carry_block_off", "y"),         # the carry product reads the state entering the PREVIOUS 32-step block
            ("pow_plus4", "y"),               # p^(k + 4) instead of p^k in the carry product
            ("mode_xor1", "y"),               # mode s read as mode s ^ 1 in the output
            ("state_early", "state"),         # the end state one step early
            ("trunc_store", "y"),             # truncation instead of round-to-nearest-even at the bf16 store
            # the single-token launches' own defects: the walks of tests/hyena_fused_exact.py are made to see them (the sweep's data does too)
            ("state_prev_row", "y"),          # the modal state of batch row m read from row m - 1
            ("chan_xor1", "y"),               # poles and residues of channel c read from channel c ^ 1 (the pair a two-channel wave owns)
            ("fir_old_kept", "y")]            # the FIR history's older column never replaced (`fir_after` gives the history it leaves)


# which family sees which mutant (U, I) after the store's rounding -- asserted on the sweep's data in tests/test_hyena_exact_host.py (the table
# with its reasons is in that module's docstring)
CAUGHT = {"fir_reversed": (True, True), "tile_hist_zero": (True, False), "row_hist_prev_row": (True, False), "swap_reim": (True, True),
          "carry_block_off": (True, True), "pow_plus4": (False, True), "mode_xor1": (True, True), "state_early": (True, True),
          "trunc_store": (True, True), "state_prev_row": (True, True), "chan_xor1": (True, True), "fir_old_kept": (True, False)}


def round_store(y, mutant=None):
    """The kernel's store: y (fp64, exactly representable in fp32) -> bf16, round-to-nearest-even."""
    if mutant == "trunc_store":
        return (y.float().contiguous().view(torch.int32) & -65536).view(torch.float32).to(BF)
    return y.to(BF)


def reference(z, prm, H, z_halo=None, s0=None, mask=None, mutant=None, state_at=None, check=None):
    """The per-step recurrence in fp64 (module docstring) -> Ref.  z [B, T, 3 D]; prm = (fir_w, fir_b, poles, residues, dskip); z_halo
    [B, 2, 3 D]: the rows before t = 0; s0 [B, D, 8] complex: the state before t = 0; mask [B, T]: 0 = pad.  state_at [B, n] int64: keep
    only these steps' states (large batches).  check "U" / "I": assert the family's exactness conditions on the way."""
    fir_w, fir_b, poles, residues, dskip = prm
    B, T, D3 = z.shape
    D, dev = D3 // 3, z.device
    zd = z.double()
    left = z_halo.double() if z_halo is not None else zd.new_zeros(B, 2, D3)
    hist = torch.cat([left, zd], 1)
    w = fir_w.double().to(dev)
    h1, h2 = hist[:, 1:T + 1].clone(), hist[:, 0:T].clone()                       # z[t - 1], z[t - 2]
    if mutant == "fir_reversed":
        w = w.flip(-1)
    if mutant == "tile_hist_zero":
        h1[:, TILE::TILE] = 0
        h2[:, TILE::TILE] = 0
    if mutant == "row_hist_prev_row" and B > 1 and T > 1:
        h1[1:, 0], h2[1:, 0] = zd[:-1, T - 1], zd[:-1, T - 2]
    if mutant == "fir_old_kept":
        h2[:] = hist[:, 0:1]
    zc = w[:, 0] * h2 + w[:, 1] * h1 + w[:, 2] * zd + fir_b.double().to(dev)
    if mask is not None:
        zc = zc * (mask != 0).double().to(dev)[:, :, None]
    x2, x1, v = _thirds(zc, H)
    x = x1 * v                                                                     # [B, T, D]
    p = torch.view_as_complex(poles.double().contiguous()).to(dev)                 # [D, 8]
    r = torch.view_as_complex(residues.double().contiguous()).to(dev)
    if mutant == "chan_xor1":
        p, r = p[torch.arange(D, device=dev) ^ 1], r[torch.arange(D, device=dev) ^ 1]
    r_out = r[:, [1, 0, 3, 2, 5, 4, 7, 6]] if mutant == "mode_xor1" else r
    S = torch.zeros(B, D, 8, dtype=torch.complex128, device=dev) if s0 is None else s0.to(torch.complex128).to(dev).clone()
    S_in = S.clone()
    keep_all = state_at is None
    n_keep = T if keep_all else state_at.shape[1]
    states = torch.zeros(B, n_keep, D, 8, dtype=torch.complex128, device=dev)
    keep = {}
    if not keep_all:
        for bi, row in enumerate(state_at.tolist()):
            for ni, t in enumerate(row):
                keep.setdefault(t, []).append((bi, ni))
    conv = torch.empty(B, T, D, dtype=torch.float64, device=dev)
    bad = torch.zeros((), dtype=torch.bool, device=dev)
    s_max = torch.zeros((), dtype=torch.float64, device=dev)
    for t in range(T):
        if mutant == "state_prev_row":
            S = torch.cat([S[:1], S[:-1]], 0)
        S = p * S + x[:, t, :, None]
        So = S
        if mutant == "swap_reim":
            So = S.clone()
            So[..., 3] = torch.complex(S[..., 3].imag, S[..., 3].real)
        conv[:, t] = (r_out * So).real.sum(-1)
        if keep_all:
            states[:, t] = S
        else:
            for bi, ni in keep.get(t, ()):
                states[bi, ni] = S[bi]
        if check is not None:
            Sr = torch.view_as_real(S)
            s_max = torch.maximum(s_max, Sr.abs().max())
            if check == "U":
                bad = bad | (Sr != Sr.round()).any()
            else:
                bad = bad | (~sig_bits_ok(torch.where(Sr.abs() >= FLUSH, Sr, torch.zeros_like(Sr)), 16)).any()
    if mutant in ("carry_block_off", "pow_plus4"):
        assert keep_all
        pw = [torch.ones_like(p)]
        for _ in range(BLOCK + 4):
            pw.append(pw[-1] * p)                                                  # exact on both families' poles
        pw = torch.stack(pw, -1)                                                   # [D, 8, 37]
        start = torch.cat([S_in[:, None], states[:, BLOCK - 1::BLOCK]], 1)         # the state entering block a
        for t in range(T):
            a, i = divmod(t, BLOCK)
            if mutant == "pow_plus4":
                d = (r * (pw[..., i + 5] - pw[..., i + 1]) * start[:, a]).real.sum(-1)
            else:
                d = (r * pw[..., i + 1] * (start[:, a - 1] - start[:, a])).real.sum(-1) if a else 0.0
            conv[:, t] += d
    if mutant == "state_early":
        assert keep_all
        states = torch.cat([S_in[:, None], states[:, :-1]], 1)
    pre = conv + dskip.double().to(dev) * x
    y = pre * x2
    if check == "U":
        assert not bool(bad) and float(s_max) < 2.0 ** 16, ("U: states must be Gaussian integers below 2^16", float(s_max))
        assert float(x.abs().max()) < 2.0 ** 8
        y8 = 8.0 * y
        assert bool((y8 == y8.round()).all()) and float(y8.abs().max()) < 2.0 ** 24 and float((8.0 * pre).abs().max()) < 2.0 ** 24
    elif check == "I":
        assert not bool(bad), "I: a state component needs more than 16 bits"
        big = y.abs() >= FLUSH
        assert bool(sig_bits_ok(torch.where(big, y, torch.zeros_like(y)), 16).all()) and bool((x2 == 1).all())
        exact = big | (y == 0)
        if s0 is not None:                                                         # s0's own response, long below fp32's smallest denormal when the
            exact = exact | (y.abs() < 2.0 ** -149)                                # first impulse comes: no fp32 number holds it (flush rule all the same)
        imp = x != 0
        if T >= 97:                                                                # lags 0 .. 96 of some impulse inside the exact region
            run = torch.cumsum((~exact).double(), 1)
            run = torch.cat([run.new_zeros(B, 1, D), run], 1)
            clean = (run[:, 97:] - run[:, :T - 96]) == 0                           # [B, T - 96, D]: steps t .. t + 96 all exact
            has, good = imp[:, :T - 96].any(1), (imp[:, :T - 96] & clean).any(1)
            assert bool((good | ~has).all()), "I: a channel has no impulse with 97 exact lags"
    return Ref(y, states, hist)


def fir_after(hist, t, mutant=None):
    """The FIR history [B, 3 D, 2] (fir_state's layout: older | newer) a single-token launch leaves behind step t, from Ref.hist."""
    old = hist[:, 0] if mutant == "fir_old_kept" else hist[:, t + 1]
    return torch.stack([old, hist[:, t + 2]], -1)


def flushed_ok(got, ref):
    """equal_or_flushed without the count (no host synchronisation) -> (ok, tiny), both bool tensors."""
    assert got.dtype == ref.dtype and got.shape == ref.shape
    tiny = (ref != 0) & (ref.double().abs() < FLUSH)
    return torch.where(tiny, got.double().abs() <= FLUSH_GOT, got == ref), tiny


def equal_or_flushed(got, ref):
    """Family I's comparison, elementwise on real tensors of one dtype: the same VALUE where ref is 0 or |ref| >= 2^-100 (ref already
    cast to got's type; the same value of one type is the same bit pattern, except that -0 == +0: the sign of an exact zero depends on
    the order of the sum and is no arithmetic), |got| <= 2^-99 in between -> (ok [bool tensor], number of elements under the flush rule)."""
    ok, tiny = flushed_ok(got, ref)
    return ok, int(tiny.sum())


# ------------------------------------------------------------------------------------------------ the families
def family_u(B, T, D, H, seed, halo=False, s0=False, device="cpu", state_at=None):
    """-> (z [B, T, 3 D] bf16, (fir_w, fir_b, poles, residues, dskip), z_halo | None, s0 | None, Ref): the exactness conditions are asserted
    on the reference run that is returned."""
    g = _gen(seed)
    z = _ri(g, -2, 2, (B, T, 3 * D)).to(BF)
    fir_w = _ri(g, -1, 1, (3 * D, 3)).to(BF)
    fir_b = _ri(g, -1, 1, (3 * D,)).to(BF)
    poles = torch.tensor(_U_POLES, dtype=torch.float32)[torch.randint(0, 4, (D, 8), generator=g)].contiguous()
    residues = (_ri(g, -2, 2, (D, 8, 2)) / 4).float().contiguous()
    dskip = (_ri(g, -2, 2, (D,)) / 2).to(BF)
    z_halo, s_in = _halo_s0(g, B, D, halo, s0)
    prm = (fir_w, fir_b, poles, residues, dskip)
    ref = reference(z, prm, H, z_halo, s_in, state_at=state_at, check="U")
    return _to(device, z, prm, z_halo, s_in, ref)


def family_i(B, T, D, H, seed, halo=False, s0=False, device="cpu", state_at=None):
    """As family_u, for family I."""
    g = _gen(seed)
    hd = D // H
    pick = torch.stack([torch.randperm(len(_I_POLES), generator=g)[:8] for _ in range(D)])          # eight DISTINCT poles per channel
    poles = torch.tensor(_I_POLES, dtype=torch.float32)[pick].contiguous()
    residues = torch.zeros(D, 8, 2)
    residues[torch.arange(D), torch.randint(0, 8, (D,), generator=g)] = \
        torch.tensor(_I_RES, dtype=torch.float32)[torch.randint(0, len(_I_RES), (D,), generator=g)]
    dskip = (torch.arange(D) % 2).to(BF)
    third = (torch.arange(3 * D) // hd) % 3                                         # 0: x2, 1: x1, 2: v
    fir_w = torch.zeros(3 * D, 3)
    fir_w[third != 0, 2] = 1.0
    fir_b = (third == 0).float()
    # impulses: per (row, channel) steps t0 < t1 < ... at least 300 apart
    first = torch.randint(320 if s0 else 0, 620 if s0 else 200, (B, D), generator=g)
    n_imp = T // 300 + 2
    steps = first[..., None] + torch.cumsum(torch.cat([torch.zeros(B, D, 1, dtype=torch.int64),
                                                       300 + torch.randint(0, 100, (B, D, n_imp - 1), generator=g)], -1), -1)
    at = torch.zeros(B, D, T + 1, dtype=torch.bool)
    at.scatter_(2, steps.clamp_max(T), torch.ones_like(steps, dtype=torch.bool))
    at = at[..., :T].transpose(1, 2)                                                # [B, T, D]
    amp = _ri(g, 1, 3, (B, T, D)) * (2 * _ri(g, 0, 1, (B, T, D)) - 1)
    x1 = torch.where(at, amp, _ri(g, -3, 3, (B, T, D)))
    vv = torch.where(at, 2 * _ri(g, 0, 1, (B, T, D)) - 1, torch.zeros(B, T, D, dtype=torch.float64))
    z5 = _ri(g, -2, 2, (B, T, H, 3, hd))
    z5[:, :, :, 1], z5[:, :, :, 2] = x1.view(B, T, H, hd), vv.view(B, T, H, hd)
    z = z5.reshape(B, T, 3 * D).to(BF)
    z_halo, s_in = _halo_s0(g, B, D, halo, s0)
    prm = (fir_w.to(BF), fir_b.to(BF), poles, residues.contiguous(), dskip)
    ref = reference(z, prm, H, z_halo, s_in, state_at=state_at, check="I")
    return _to(device, z, prm, z_halo, s_in, ref)


def _to(device, z, prm, z_halo, s0, ref):
    d = lambda t: None if t is None else t.to(device)
    return d(z), tuple(d(t) for t in prm), d(z_halo), d(s0), Ref(*(d(t) for t in ref))


FAMILIES = {"U": family_u, "I": family_i}


def make(fam, B, T, D, H, seed, halo=False, s0=False, device="cpu", state_at=None):
    return FAMILIES[fam](B, T, D, H, seed, halo=halo, s0=s0, device=device, state_at=state_at)


# ------------------------------------------------------------------------------------------------ cases (shared by the CPU and the GPU module)
VARIANTS = [(False, False), (True, False), (True, True)]                            # (z_halo, s0): plain | halo | halo + s0
SWEEP = dict(B=2, T=1040, D=128, H=1, seed=7)                                       # one reference run per family and variant
SWEEP_RANGES = [(1, 64), (480, 544), (1016, 1040)]                                  # every T in these (inclusive)
GEOMETRY = [(17, 520, 256, 2), (33, 300, 128, 1), (1, 2056, 256, 2)]                # rows sharing a workgroup; head stride; four tiles + tail form
SUBRANGE = [(5, 700, 256, 2), (5, 1026, 256, 2)]                                    # b_first / b_total: plain form | tail form
MAIN_ONLY = (2, 520, 128, 1)                                                        # tail form, r = 8, B r = 16
MODAL = [(2, 37, 128, 1), (2, 3, 128, 1), (1, 1, 128, 1), (2, 520, 256, 2)]
MODAL_SEGS = [4, 8, 64, 512, None]
STATE_AT = [(40, 320, 128, 1), (40, 768, 128, 1)]
STATE_AT_TOKEN_MAJOR = (3, 300, 128, 1)                                             # T no multiple of 64
STEP = (3, 37 + 40, 256, 2)                                                         # a prefill of 37 steps, then 40 single-token launches
CROSS = (2, 700, 128, 1)
CROSS_CUTS = [33, 512, 517]
SEED = 11


def last_step(B, T):
    """state_at of the large batches: the end state alone."""
    return torch.full((B, 1), T - 1, dtype=torch.int64)


def state_at_lens(B, T):
    """The launches of the state_at tests: [n, B] int64 lens that together take EVERY value 1 .. T (scrambled: 37 is coprime to both T)."""
    n = (T + B - 1) // B
    i = torch.arange(n * B, dtype=torch.int64).view(n, B)
    return 1 + (i * 37) % T


def gpu_cases():
    """Every (family, B, T, D, H, seed, halo, s0, state_at) whose generator runs in tests/test_gpu_hyena_exact.py."""
    out = []
    for fam in ("U", "I"):
        out += [(fam, SWEEP["B"], SWEEP["T"], SWEEP["D"], SWEEP["H"], SWEEP["seed"], h, s, None) for h, s in VARIANTS]
        out += [(fam, *shp, SEED, False, False, last_step(*shp[:2])) for shp in GEOMETRY + SUBRANGE]
        out += [(fam, *shp, SEED, False, False, None) for shp in (MAIN_ONLY, STATE_AT_TOKEN_MAJOR)]
        out += [(fam, *shp, SEED, h, s, None) for shp in MODAL for h, s in ((False, False), (True, True))]
        out += [(fam, B, T, D, H, SEED, False, False, state_at_lens(B, T).t().contiguous() - 1) for B, T, D, H in STATE_AT]
        out += [(fam, *STEP, SEED, False, False, None)]
    out += [("U", *CROSS, SEED, False, False, None)]
    return out
