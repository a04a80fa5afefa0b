"""GPU (-m gpu): the Hyena operator on EXACT sums (tests/hyena_exact.py; PARITY row 9d) -- every launch form against the per-step fp64
recurrence, with no tolerance term.

Families U (unit poles, integer data: every state a Gaussian integer below 2^16, every output a multiple of 1 / 8 below 2^21) and I (dyadic
decaying poles, sparse impulses: every output one product R p^(t - t0) a) make the operator's arithmetic exact in fp32 in any order of
summation and through the bf16 hi + lo operand splits of csrc/hyena_ct.hip (tests/test_hyena_exact_host.py: the CPU emulation of those
precisions equals the reference before the output rounding, 0 differing elements).  So:
  y        == reference(...).y rounded ONCE to bf16 (round-to-nearest-even; a third of U's outputs are rounded, many on exact ties)
  states   == reference(...).states cast to complex64 (integers / dyadics below 2^24: the cast is exact)
as VALUES of the same type -- the same bit pattern, except that -0 == +0 (the sign of an exact zero depends on the order of a sum).  NaN
equals nothing.  Family I only: where 0 < |ref| < 2^-100 (fp32 flushes: decayed tails) the rule is |got| <= 2^-99, never a skip.  Every
launch is issued twice and the pair must hold the same BITS.  Pad and tail-block slack of z^T is NaN (zt_from_rows(..., nan)); output
buffers are pre-filled with a sentinel wherever a form leaves rows untouched.  table_ok is False for family I's filters; that guard is
the model's routing, HipOps.hyena_ct does not consult it.

  a  hyena_ct, every T in 1 .. 64, 480 .. 544, 1016 .. 1040 (B = 2: every (block, local step) of the end-state walk, the tile seam, the
     tail form of z^T at r = 1 .. 8 with B r = 16 at r = 8, the padded form from r = 9, both again in the third tile) x {plain, z_halo,
     z_halo + s0} x {want_state, no state, state_only, blocked y at y_row0 = 77}
  b  hyena_ct geometry: rows that share a workgroup (B = 17 and 33), the head stride (H = 2), four tiles + the tail form, b_first /
     b_total sub-ranges, main_only + the tail tokens through hyena_step
  c  the modal three-launch form (hyena_prefill) over seg_len, with halo + s0, with a padding mask; stage1 / stage2 (carry_add)
  d  hyena_state_at_zt / hyena_state_at: lens takes EVERY value 1 .. T
  e  evo_hyena_step: 40 launches in a row from the prefill's state
  f  a sequence cut in two, one piece per form, both orders
"""
import pytest
import torch

import hyena_exact as X

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BF = torch.bfloat16
NAN = float("nan")
SENT = 7.0
COUNT = {"launches": 0, "lens": 0, "tiny": 0, "nonzero": 0}


@pytest.fixture(scope="module")
def ops():
    from evo_amd.ops import HipOps
    return HipOps()


class Case:
    """One data set on the device: z, the parameters, halo / s0 (or None), the reference, the operand table of hyena_ct."""
    _cache = {}

    def __init__(self, fam, B, T, D, H, seed, halo=False, s0=False, state_at=None):
        from evo_amd.hyena_tables import mfma_operand_table
        self.fam, self.B, self.T, self.D, self.H = fam, B, T, D, H
        self.z, self.prm, self.halo, self.s0, self.ref = X.make(fam, B, T, D, H, seed, halo=halo, s0=s0, device=DEV, state_at=state_at)
        self.fir_w, self.fir_b, self.poles, self.res, self.dskip = self.prm
        self.tab = mfma_operand_table(self.poles, self.res, self.dskip)
        self.kw = {k: v for k, v in (("z_halo", self.halo), ("s0", self.s0)) if v is not None}

    @classmethod
    def get(cls, fam, B, T, D, H, seed, halo=False, s0=False, state_at=None):
        key = (fam, B, T, D, H, seed, halo, s0, None if state_at is None else tuple(state_at.shape))
        if key not in cls._cache:
            cls._cache[key] = cls(fam, B, T, D, H, seed, halo, s0, state_at)
        return cls._cache[key]


def _bits(t):
    if t.is_complex():
        t = torch.view_as_real(t)
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def _twice(fn):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for x, y in zip(a if isinstance(a, tuple) else (a,), b if isinstance(b, tuple) else (b,)):
        assert torch.equal(_bits(x), _bits(y)), "two launches differ"
    return a


def _same(got, ref, fam, what, count=True):
    """got == ref as values of got's type (module docstring); family I: the flush rule in the tiny region."""
    if got.is_complex():
        got, ref = torch.view_as_real(got), torch.view_as_real(ref.to(got.dtype))
    else:
        ref = ref.to(got.dtype)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if fam == "U":
        ok = got == ref
    else:
        ok, n_tiny = X.equal_or_flushed(got, ref)
        if count:
            COUNT["tiny"] += n_tiny
            COUNT["nonzero"] += int((ref != 0).sum())
    if not bool(ok.all()):
        bad = (~ok).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {bad.shape[0]} of {ok.numel()} elements differ; first at {i}: got {got[i].item()!r}, reference {ref[i].item()!r}")


def _ct(ops, c, zt, B, T, **kw):
    return ops.hyena_ct(zt, B, T, c.fir_w, c.fir_b, c.tab, c.H, **kw)


def _blocked(ops, c, zt, B, T, rows_y, **kw):
    """The blocked-y form at y_row0 = 77 -> the [B, T, D] rows it wrote; everything else in the buffer keeps the sentinel."""
    def run():
        yb = ops.yblk_empty(B * T + 77, c.D, DEV).fill_(SENT)
        _ct(ops, c, zt, B, T, y_blk=yb, y_row0=77, **kw)
        return ops.yblk_to_rows(yb, yb.shape[0] * ops.YBLK)
    rows = _twice(run)
    assert bool((rows[:77] == SENT).all()) and bool((rows[77 + rows_y:] == SENT).all()), "blocked y: rows outside the launch were written"
    return rows[77:77 + rows_y]


def _all_forms(ops, c, T, what, rows=None, kw=None):
    """Every launch form of hyena_ct on the first T steps of c's batch rows `rows` (default: all) against the reference -> launches made."""
    kw = c.kw if kw is None else kw
    b0, b1 = rows or (0, c.B)
    B = b1 - b0
    z = c.z[b0:b1, :T].contiguous()
    kw = {k: v[b0:b1].contiguous() for k, v in kw.items()}
    zt = ops.zt_from_rows(z, B, T, NAN)
    ref_y = X.round_store(c.ref.y[b0:b1, :T])
    ref_s = c.ref.states[b0:b1, T - 1 if c.ref.states.shape[1] == c.T else -1]
    y, s = _twice(lambda: _ct(ops, c, zt, B, T, want_state=True, poles=c.poles, **kw))
    _same(y, ref_y, c.fam, f"{what}: y (want_state)")
    _same(s, ref_s, c.fam, f"{what}: end state")
    y_pln = _twice(lambda: _ct(ops, c, zt, B, T, **kw))
    assert torch.equal(_bits(y_pln), _bits(y)), f"{what}: the no-state form differs from the want_state form"
    s_only = _twice(lambda: _ct(ops, c, zt, B, T, poles=c.poles, state_only=True, **kw))
    assert torch.equal(_bits(s_only), _bits(s)), f"{what}: the state_only form differs"
    y_blk = _blocked(ops, c, zt, B, T, B * T, **kw)
    assert torch.equal(_bits(y_blk.view(B, T, c.D)), _bits(y)), f"{what}: the blocked form differs"
    return 8


# ================================================================================================ a. hyena_ct, sweep of T
@pytest.mark.parametrize("t_range", X.SWEEP_RANGES)
@pytest.mark.parametrize("variant", range(len(X.VARIANTS)))
@pytest.mark.parametrize("fam", ["U", "I"])
def test_ct_sweep_of_T(ops, fam, variant, t_range):
    halo, s0 = X.VARIANTS[variant]
    c = Case.get(fam, X.SWEEP["B"], X.SWEEP["T"], X.SWEEP["D"], X.SWEEP["H"], X.SWEEP["seed"], halo, s0)
    n, forms = 0, set()
    for T in range(t_range[0], t_range[1] + 1):
        n += _all_forms(ops, c, T, f"{fam} T {T} halo {halo} s0 {s0}")
        forms.add(ops.zt_layout(c.B, T)[3])
    COUNT["launches"] += n
    if t_range[0] >= 480:
        assert forms == set(range(9)), forms                     # the tail form at r = 1 .. 8 and the plain form on both sides of it
    print(f"[hyena exact] sweep {fam} T {t_range} halo {halo} s0 {s0}: {n} launches ({n // 2} (T, variant, form) twice); so far {COUNT['launches']}")


@pytest.mark.parametrize("fam", ["U", "I"])
def test_ct_output_is_no_mutants(ops, fam):
    """The comparison has teeth: at T = 1,040 with z_halo + s0 the kernel's y / end state, equal to the reference above, differs under the
    same rule from every deliberately wrong reference this family sees (X.CAUGHT, asserted on the same data on the CPU)."""
    c = Case.get(fam, X.SWEEP["B"], X.SWEEP["T"], X.SWEEP["D"], X.SWEEP["H"], X.SWEEP["seed"], True, True)
    zt = ops.zt_from_rows(c.z, c.B, c.T, NAN)
    y, s = _ct(ops, c, zt, c.B, c.T, want_state=True, poles=c.poles, **c.kw)
    _same(y, X.round_store(c.ref.y), fam, "y")
    n = 0
    for name, what in X.mutants():
        if not X.CAUGHT[name][("U", "I").index(fam)]:
            continue
        mut = c.ref if name == "trunc_store" else X.reference(c.z.cpu(), [t.cpu() for t in c.prm], c.H, c.halo.cpu(), c.s0.cpu(), mutant=name)
        with pytest.raises(AssertionError, match="elements differ"):
            if what == "y":
                _same(y, X.round_store(mut.y, name).to(DEV), fam, name, count=False)
            else:
                _same(s, mut.states[:, -1].to(DEV), fam, name, count=False)
        n += 1
    assert n >= 7


# ================================================================================================ b. hyena_ct, geometry
@pytest.mark.parametrize("B,T,D,H", X.GEOMETRY)
@pytest.mark.parametrize("fam", ["U", "I"])
def test_ct_geometry(ops, fam, B, T, D, H):
    c = Case.get(fam, B, T, D, H, X.SEED, False, False, X.last_step(B, T))
    _all_forms(ops, c, T, f"{fam} {B} x {T} x {D}")


@pytest.mark.parametrize("B,T,D,H", X.SUBRANGE)
@pytest.mark.parametrize("fam", ["U", "I"])
def test_ct_row_subrange(ops, fam, B, T, D, H):
    """b_first / b_total: rows 3 .. 4 of the five-row tensor; a three-row tensor of rows 1 .. 3 (another layout of the same rows)."""
    c = Case.get(fam, B, T, D, H, X.SEED, False, False, X.last_step(B, T))
    zt = ops.zt_from_rows(c.z, B, T, NAN)
    y, s = _twice(lambda: _ct(ops, c, zt, 2, T, b_first=3, b_total=B, want_state=True, poles=c.poles))
    _same(y, X.round_store(c.ref.y[3:5]), fam, "sub-range y")
    _same(s, c.ref.states[3:5, -1], fam, "sub-range end state")
    _all_forms(ops, c, T, f"{fam} rows 1 .. 3 of {B} x {T} x {D}", rows=(1, 4))
    assert torch.equal(_bits(ops.zt_rows(zt, B, T, T - 2, 2)), _bits(c.z[:, T - 2:]))


@pytest.mark.parametrize("fam", ["U", "I"])
def test_ct_main_only_then_the_tail_tokens_by_single_steps(ops, fam):
    """main_only on a tail-form shape (r = 8, B r = 16): y rows T_m .. T - 1 untouched, the state after T_m - 1, then the tail tokens
    through hyena_step from that state."""
    B, T, D, H = X.MAIN_ONLY
    c = Case.get(fam, B, T, D, H, X.SEED, False, False, None)
    Tm, _, _, r = ops.zt_layout(B, T)
    assert (Tm, r) == (512, 8)
    zt = ops.zt_from_rows(c.z, B, T, NAN)

    def run():
        yb = ops.yblk_empty(B * T + 77, D, DEV).fill_(SENT)
        _, st = _ct(ops, c, zt, B, T, y_blk=yb, y_row0=77, main_only=True, want_state=True, poles=c.poles)
        return ops.yblk_to_rows(yb, yb.shape[0] * ops.YBLK), st
    rows, st = _twice(run)
    y = rows[77:77 + B * T].view(B, T, D)
    _same(y[:, :Tm], X.round_store(c.ref.y[:, :Tm]), fam, "main_only y")
    assert bool((y[:, Tm:] == SENT).all()) and bool((rows[:77] == SENT).all()) and bool((rows[77 + B * T:] == SENT).all())
    _same(st, c.ref.states[:, Tm - 1], fam, "main_only state")
    _steps(ops, c, st.clone(), Tm, T)


def _steps(ops, c, st, t0, t1):
    """hyena_step for the steps t0 .. t1 - 1 from the state `st` after t0 - 1; y, fir_state and iir_state after EVERY step."""
    fs = c.ref.hist[:, t0:t0 + 2].transpose(1, 2).to(BF).contiguous()
    st2, fs2 = st.clone(), fs.clone()
    for t in range(t0, t1):
        z_t = c.z[:, t].contiguous()
        y = ops.hyena_step(z_t, fs, st, c.fir_w, c.fir_b, c.poles, c.res, c.dskip, c.H)
        y2 = ops.hyena_step(z_t, fs2, st2, c.fir_w, c.fir_b, c.poles, c.res, c.dskip, c.H)
        assert torch.equal(_bits(y), _bits(y2)) and torch.equal(_bits(fs), _bits(fs2)) and torch.equal(_bits(st), _bits(st2)), t
        _same(y, X.round_store(c.ref.y[:, t]), c.fam, f"step {t}: y")
        _same(fs, c.ref.hist[:, t + 1:t + 3].transpose(1, 2), "U", f"step {t}: fir_state")
        _same(st, c.ref.states[:, t], c.fam, f"step {t}: iir_state")


# ================================================================================================ c. the modal three-launch form
def _prefill(ops, c, z, **kw):
    return ops.hyena_prefill(z, c.fir_w, c.fir_b, c.poles, c.res, c.dskip, c.H, want_state=True, **kw)


@pytest.mark.parametrize("with_state", [False, True])
@pytest.mark.parametrize("B,T,D,H", X.MODAL)
@pytest.mark.parametrize("fam", ["U", "I"])
def test_modal_form_over_segment_lengths(ops, fam, B, T, D, H, with_state):
    c = Case.get(fam, B, T, D, H, X.SEED, with_state, with_state, None)
    for seg in X.MODAL_SEGS:
        y, s = _twice(lambda: _prefill(ops, c, c.z, seg_len=seg, **c.kw))
        _same(y, X.round_store(c.ref.y), fam, f"modal seg {seg}: y")
        _same(s, c.ref.states[:, -1], fam, f"modal seg {seg}: end state")


@pytest.mark.parametrize("fam", ["U", "I"])
def test_modal_form_with_padding_mask(ops, fam):
    """Pads at step 0, across a segment seam (62 .. 66: the seams of seg_len 8 and 64) and at the end."""
    B, T, D, H = X.MODAL[3]
    c = Case.get(fam, B, T, D, H, X.SEED, False, False, None)
    mask = torch.ones(B, T, dtype=torch.bool, device=DEV)
    mask[0, 0] = False
    mask[0, 62:67] = False
    mask[1, T - 20:] = False
    ref = X.reference(c.z, c.prm, H, mask=mask)
    for seg in (8, 64, None):
        y, s = _twice(lambda: _prefill(ops, c, c.z, seg_len=seg, mask=mask))
        _same(y, X.round_store(ref.y), fam, f"mask seg {seg}: y")
        _same(s, ref.states[:, -1], fam, f"mask seg {seg}: end state")
        assert bool((y[0, 62:67] == 0).all()) and bool((y[1, T - 20:] == 0).all()) and bool((y[0, 0] == 0).all())


@pytest.mark.parametrize("fam", ["U", "I"])
def test_modal_two_stage_form_with_carry_add(ops, fam):
    """hyena_stage1 (the end state from a ZERO carry-in) then hyena_stage2 with a non-zero s0 (evo_hyena_carry_add)."""
    B, T, D, H = X.MODAL[3]
    c = Case.get(fam, B, T, D, H, X.SEED, True, True, None)
    zero_in = X.reference(c.z, c.prm, H, z_halo=c.halo)
    for seg in (8, 64, None):
        def run():
            st1, s_end = ops.hyena_stage1(c.z, c.fir_w, c.fir_b, c.poles, H, z_halo=c.halo, seg_len=seg)
            return ops.hyena_stage2(c.z, c.fir_w, c.fir_b, c.poles, c.res, c.dskip, H, st1, z_halo=c.halo, s0=c.s0), s_end
        y, s_end = _twice(run)
        _same(s_end, zero_in.states[:, -1], fam, f"stage1 seg {seg}: end state from a zero start")
        _same(y, X.round_store(c.ref.y), fam, f"stage2 seg {seg}: y")


# ================================================================================================ d. the ragged end states
@pytest.mark.parametrize("B,T,D,H", X.STATE_AT)
@pytest.mark.parametrize("fam", ["U", "I"])
def test_state_at_every_length(ops, fam, B, T, D, H):
    """lens takes every value 1 .. T over the launches; positions at and behind lens[b] hold NaN.  s_out == the reference's state after
    step lens[b] - 1, fir_out == the two rows of z there (zeros in front of t = 0)."""
    lens_all = X.state_at_lens(B, T)
    c = Case.get(fam, B, T, D, H, X.SEED, False, False, lens_all.t().contiguous() - 1)
    steps = torch.arange(T, device=DEV)
    for k, lens in enumerate(lens_all.to(DEV)):
        zn = torch.where((steps[None, :] < lens[:, None])[:, :, None], c.z, torch.full_like(c.z, NAN))
        zt = ops.zt_from_rows(zn, B, T, NAN)
        st, fir = _twice(lambda: ops.hyena_state_at_zt(zt, B, T, lens, c.fir_w, c.fir_b, c.poles, H))
        _same(st, c.ref.states[:, k], fam, f"state_at_zt launch {k}")
        idx = (lens[:, None] + torch.arange(2, device=DEV)[None, :])                 # hist rows lens .. lens + 1 = z rows lens - 2, lens - 1
        want = c.ref.hist[torch.arange(B, device=DEV)[:, None], idx].transpose(1, 2)
        _same(fir, want, "U", f"state_at_zt launch {k}: fir_out")
        COUNT["lens"] += B
    print(f"[hyena exact] state_at {fam} {B} x {T}: {lens_all.numel()} lens in {lens_all.shape[0]} launches, every value 1 .. {T}; so far {COUNT['lens']}")


@pytest.mark.parametrize("fam", ["U", "I"])
def test_state_at_token_major(ops, fam):
    """hyena_state_at on token-major z whose T is no multiple of 64."""
    B, T, D, H = X.STATE_AT_TOKEN_MAJOR
    c = Case.get(fam, B, T, D, H, X.SEED, False, False, None)
    lens = torch.tensor([T, 1, 257], dtype=torch.int64, device=DEV)
    st, fir = _twice(lambda: ops.hyena_state_at(c.z, lens, c.fir_w, c.fir_b, c.poles, H))
    rows = torch.arange(B, device=DEV)
    _same(st, c.ref.states[rows, lens - 1], fam, "state_at (token-major)")
    want = c.ref.hist[rows[:, None], lens[:, None] + torch.arange(2, device=DEV)[None, :]].transpose(1, 2)
    _same(fir, want, "U", "state_at (token-major): fir_out")


# ================================================================================================ e. single steps
@pytest.mark.parametrize("fam", ["U", "I"])
def test_forty_single_steps_from_the_prefills_state(ops, fam):
    B, T, D, H = X.STEP
    c = Case.get(fam, B, T, D, H, X.SEED, False, False, None)
    T0 = T - 40
    _, st = _prefill(ops, c, c.z[:, :T0].contiguous())
    _same(st, c.ref.states[:, T0 - 1], fam, "prefill state")
    _steps(ops, c, st.clone(), T0, T)


# ================================================================================================ f. one sequence, two forms
@pytest.mark.parametrize("cut", X.CROSS_CUTS)
def test_sequence_cut_in_two_one_piece_per_form(ops, cut):
    B, T, D, H = X.CROSS
    c = Case.get("U", B, T, D, H, X.SEED, False, False, None)
    za, zb, halo = c.z[:, :cut].contiguous(), c.z[:, cut:].contiguous(), c.z[:, cut - 2:cut].contiguous()
    ref_y = X.round_store(c.ref.y)

    def ct(z, **kw):
        Bz, Tz, _ = z.shape
        return _twice(lambda: _ct(ops, c, ops.zt_from_rows(z, Bz, Tz, NAN), Bz, Tz, want_state=True, poles=c.poles, **kw))

    def modal(z, **kw):
        return _twice(lambda: _prefill(ops, c, z, **kw))
    for first, second, what in ((ct, modal, "hyena_ct then modal"), (modal, ct, "modal then hyena_ct")):
        ya, sa = first(za)
        _same(sa, c.ref.states[:, cut - 1], "U", f"{what}: state at the cut")
        yb, sb = second(zb, z_halo=halo, s0=sa)
        _same(torch.cat([ya, yb], 1), ref_y, "U", f"{what}: y")
        _same(sb, c.ref.states[:, -1], "U", f"{what}: end state")


def test_counts():
    """The run's totals (for the record; the tests above assert)."""
    share = 100.0 * COUNT["tiny"] / max(1, COUNT["nonzero"])
    print(f"[hyena exact] totals: {COUNT['launches']} sweep launches = {COUNT['launches'] // 2} (T, variant, form) combinations, each twice; "
          f"{COUNT['lens']} lens values; family I: {COUNT['tiny']} of {COUNT['nonzero']} non-zero reference elements compared under the "
          f"flush rule ({share:.1f} %)")
