"""GPU (-m gpu): beam search on the device -- the selection kernel `evo_beam_select_f32` against the written
specification (evo_amd/sh/sample.py: beam_select), the reparenting copy `evo_gather_rows` against `index_select`, and
`DecodePool.beam_search` on the toy model.

Selection.  The kernel ranks f32 scores, the specification fp64 ones, so the test asserts an INPUT CONDITION in fp64 before any launch:
among the best W + 1 candidates of every active group any two scores differ by more than 2^-10 (the f32 error of a score below 64 in
magnitude is some 2^-17: the ranking is then decided), except two candidates of one parent with bit-equal logits, which tie exactly in f32
too and are ordered by token.  The seeds below were chosen on the CPU for that condition; no case is left out.  parent / ids / ended /
length / the history must then be EQUAL; cum is held to 4 x the error of the same formula in fp32 torch (the rule of
tests/test_gpu_sample.py), over all the sizes of a sweep together.

Pool.  (b) is the end-to-end check that states and keys moved with the hypotheses: every returned hypothesis is generated again by a
sampling pool of the same shape, forced token by token through an IUPAC template; its log-probabilities summed in f32 in step order must
equal the hypothesis's score BIT FOR BIT (tests/PARITY_beam.md)."""
import pytest
import torch

from evo_amd.sh import sample as H
from test_gpu_arena import _run, covers, gen, is_poison, poisoned, rnd
from test_gpu_model import DEV, SMALL4, build
from test_gpu_pool import PROMPTS
from test_gpu_sample import acgt_mask, ops

pytestmark = pytest.mark.gpu
NEG = float("-inf")
GAP = 2.0 ** -10
STOP_IDS = (ord("G"), 7, 300)
CANARY = 8
# (W, G) -> seed for which the input condition holds in all four (dtype, mask) variants of both kinds (chosen on the CPU)
SIZES = [(1, 1), (2, 1), (3, 1), (4, 1), (8, 1), (1, 3), (2, 3), (3, 3), (4, 3), (8, 3)]
SEEDS = {(1, 1): 0, (2, 1): 0, (3, 1): 0, (4, 1): 0, (8, 1): 0, (1, 3): 0, (2, 3): 0, (3, 3): 0, (4, 3): 0, (8, 3): 0}


def stop_mask():
    m = torch.zeros(512, dtype=torch.bool)
    m[list(STOP_IDS)] = True
    return m


def make_case(W, G, seed, kind):
    """S = G W + 1 slots (one leftover; with W = 1 there is none: S = G).  "mixed": random cum, beam 1 of a group ended, beam 2 empty, group 1 of three inactive, a -inf
    logit in every row; "seed": the admission state cum = [0, -inf, ...]."""
    g = torch.Generator().manual_seed(1000 * seed + 10 * W + G)
    S = G * W + (1 if W > 1 else 0)
    x = (torch.randn(S, 512, generator=g) * 3).bfloat16()
    x[:, 11] = NEG
    ids = torch.randint(0, 512, (S,), generator=g)
    length = torch.randint(0, 50, (S,), generator=g)
    ended = torch.zeros(S, dtype=torch.uint8)
    active = torch.ones(G, dtype=torch.uint8)
    if kind == "seed":
        cum = torch.full((S,), NEG)
        cum[torch.arange(G) * W] = 0.0
        length.zero_()
    else:
        cum = -(torch.rand(S, generator=g) * 20)
        for q in range(G):
            if W >= 2:
                ended[q * W + 1] = 1
                ids[q * W + 1] = ord("C") if q % 2 else 300           # (an ended beam's token may be a stop token: it is not looked at)
            if W >= 3:
                cum[q * W + 2] = NEG
        if G == 3:
            active[1] = 0
    return x, cum.float(), ended, length, ids, active


def candidates(x, cum, ended, ids, W, q, mask):
    """fp64 candidates of group q: [(score, parent, token, logit bits)]."""
    out = []
    for b in range(q * W, q * W + W):
        if not cum[b] > NEG:
            continue
        if ended[b]:
            out.append((float(cum[b]), b, int(ids[b]), None))
            continue
        row = x[b].double()
        sc = cum[b].double() + (row - torch.logsumexp(row, -1))
        for v in range(512):
            if (mask is None or mask[v]) and sc[v] > NEG:
                out.append((float(sc[v]), b, v, float(row[v])))
    return out


def condition_holds(x, cum, ended, ids, active, W, mask):
    for q in range(active.numel()):
        if not active[q]:
            continue
        c = sorted(candidates(x, cum, ended, ids, W, q, mask), key=lambda t: (-t[0], t[1], t[2]))[:W + 1]
        for i in range(len(c)):
            for j in range(i + 1, len(c)):
                same = c[i][1] == c[j][1] and c[i][3] is not None and c[i][3] == c[j][3]
                if abs(c[i][0] - c[j][0]) <= GAP and not same:
                    return False
    return True


def guarded(t, fill):
    """`t` on the device inside a buffer with CANARY cells of `fill` on either side -> (view, buffer)."""
    buf = torch.full((t.numel() + 2 * CANARY,), fill, dtype=t.dtype, device=DEV)
    view = buf[CANARY:CANARY + t.numel()].view(t.shape)
    view.copy_(t.to(DEV))
    return view, buf


def guards_stand(buf, fill):
    return bool((buf[:CANARY] == fill).all()) and bool((buf[-CANARY:] == fill).all())


def launch(x, cum, ended, length, ids, active, W, f32, mask, stop, L=5, col=3):
    S = x.shape[0]
    st = {"cum": guarded(cum, 77.0), "ended": guarded(ended, 9), "length": guarded(length, -5), "ids": guarded(ids, -6),
          "parent": guarded(torch.full((S,), -3, dtype=torch.int64), -4),
          "hp": guarded(torch.full((S, L), -8, dtype=torch.int32), -9), "hi": guarded(torch.full((S, L), -10, dtype=torch.int64), -11),
          "hc": guarded(torch.full((S, L), 55.0), 66.0)}
    o = ops()
    o.beam_select((x.float() if f32 else x).to(DEV), st["cum"][0], st["ended"][0], st["length"][0], st["ids"][0], st["parent"][0], W,
                  group_active=active.to(DEV), allow=None if mask is None else o.pack_allow_mask(mask, DEV),
                  stop_mask=None if stop is None else o.pack_allow_mask(stop, DEV), hist_parent=st["hp"][0], hist_ids=st["hi"][0],
                  hist_cum=st["hc"][0], t=col)
    torch.cuda.synchronize()
    fills = {"cum": 77.0, "ended": 9, "length": -5, "ids": -6, "parent": -4, "hp": -9, "hi": -11, "hc": 66.0}
    for k, (_, buf) in st.items():
        assert guards_stand(buf, fills[k]), k
    return {k: v[0].cpu() for k, v in st.items()}


def check_against_spec(x, cum, ended, length, ids, active, W, f32, mask, stop, got, L=5, col=3):
    """Everything but cum EQUAL to the specification; -> (kernel |err|, fp32 torch |err|) of cum over the slots that received a live candidate."""
    S, G = x.shape[0], active.numel()
    p, i, c, e, n = H.beam_select(x, cum, ended, length, ids, W, active, mask, stop, dtype=torch.float64)
    assert torch.equal(got["parent"][:G * W], p[:G * W]) and torch.equal(got["ids"], i) and torch.equal(got["length"], n)
    assert torch.equal(got["ended"].bool(), e)
    assert torch.equal(got["parent"][G * W:], torch.arange(G * W, S))  # the leftover slot
    assert torch.equal(torch.isinf(got["cum"]), torch.isinf(c)) and not bool(torch.isnan(got["cum"]).any())
    rows = torch.cat([torch.arange(q * W, q * W + W) for q in range(G) if active[q]])
    hp, hi, hc = torch.full((S, L), -8, dtype=torch.int32), torch.full((S, L), -10, dtype=torch.int64), torch.full((S, L), 55.0)
    hp[rows, col], hi[rows, col], hc[rows, col] = p[rows].int(), i[rows], got["cum"][rows]
    assert torch.equal(got["hp"], hp) and torch.equal(got["hi"], hi) and torch.equal(got["hc"], hc)      # and nothing else of the history
    idle = torch.ones(S, dtype=torch.bool)
    idle[rows] = False
    assert torch.equal(got["cum"][idle], cum[idle])                    # inactive groups and the leftover slot: untouched
    live = [s for s in rows.tolist() if c[s] > NEG and not ended[p[s]]]
    if not live:
        return 0.0, 0.0
    live = torch.tensor(live)
    x32 = x.float()
    mx = x32.max(-1, keepdim=True)[0]
    lse32 = (mx + (x32 - mx).exp().sum(-1, keepdim=True).log())[:, 0]
    ref32 = cum[p[live]] + (x32[p[live], i[live]] - lse32[p[live]])
    carried = [s for s in rows.tolist() if c[s] > NEG and ended[p[s]]]
    assert all(got["cum"][s] == cum[p[s]] for s in carried)            # an ended beam's score is carried, not recomputed
    return (got["cum"][live].double() - c[live]).abs().max().item(), (ref32.double() - c[live]).abs().max().item()


@pytest.mark.parametrize("kind", ["mixed", "seed"])
@pytest.mark.parametrize("masked", [False, True], ids=["all", "acgt"])
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
def test_select_kernel_equals_the_specification(f32, masked, kind):
    mask, stop = (acgt_mask() if masked else None), stop_mask()
    err = err32 = 0.0
    for W, G in SIZES:
        x, cum, ended, length, ids, active = make_case(W, G, SEEDS[(W, G)], kind)
        assert condition_holds(x, cum, ended, ids, active, W, mask), (W, G)       # the input condition, in fp64, before the kernel runs
        got = launch(x, cum, ended, length, ids, active, W, f32, mask, stop)
        a, b = check_against_spec(x, cum, ended, length, ids, active, W, f32, mask, stop, got)
        err, err32 = max(err, a), max(err32, b)
    print(f"[beam select f32={f32} acgt={masked} {kind}] cum: kernel max |err| {err:.3e}, fp32 torch restatement {err32:.3e}")
    assert err <= 4 * err32, (err, err32)


def test_select_kernel_ties_nan_and_too_few_candidates():
    mask = acgt_mask()
    # (1) exact ties across parents: four equal rows with equal cum -- parent ascending decides, then the token
    W, S = 4, 5
    row = (torch.randn(512, generator=torch.Generator().manual_seed(5)) * 3).bfloat16()
    row[ord("A")] = row[ord("C")] = 9.0                                # ... and two bit-equal logits within a row
    x = row[None].repeat(S, 1)
    cum, ended = torch.full((S,), -1.5), torch.zeros(S, dtype=torch.uint8)
    length, ids, active = torch.zeros(S, dtype=torch.int64), torch.zeros(S, dtype=torch.int64), torch.ones(1, dtype=torch.uint8)
    for f32 in (False, True):
        got = launch(x, cum, ended, length, ids, active, W, f32, mask, None)
        check_against_spec(x, cum, ended, length, ids, active, W, f32, mask, None, got)
        assert got["parent"][:4].tolist() == [0, 0, 1, 1] and got["ids"][:4].tolist() == [ord("A"), ord("C"), ord("A"), ord("C")]
        assert len(set(got["cum"][:4].tolist())) == 1
    # (2) a NaN logit: the row's log-sum-exp is NaN, the beam offers nothing; the one live beam left has A, C, G (its T is -inf): three
    # candidates for 8 slots, the other five become empty
    W, S = 8, 9
    x = (torch.randn(S, 512, generator=torch.Generator().manual_seed(6)) * 3).bfloat16()
    x[0, 200] = float("nan")
    x[1, ord("T")] = NEG
    cum = torch.full((S,), NEG)
    cum[0], cum[1] = -0.5, -2.0
    ended, length, ids = torch.zeros(S, dtype=torch.uint8), torch.full((S,), 3, dtype=torch.int64), torch.arange(S) + 40
    assert condition_holds(x, cum, ended, ids, torch.ones(1, dtype=torch.uint8), W, mask)
    for f32 in (False, True):
        got = launch(x, cum, ended, length, ids, torch.ones(1, dtype=torch.uint8), W, f32, mask, stop_mask())
        check_against_spec(x, cum, ended, length, ids, torch.ones(1, dtype=torch.uint8), W, f32, mask, stop_mask(), got)
        assert got["parent"][:8].tolist() == [1, 1, 1, 3, 4, 5, 6, 7] and bool(torch.isinf(got["cum"][3:8]).all())
        assert sorted(got["ids"][:3].tolist()) == sorted(ord(c) for c in "ACG") and got["ids"][3:8].tolist() == [43, 44, 45, 46, 47]
        assert got["ended"][:3].tolist() == [int(t == ord("G")) for t in got["ids"][:3].tolist()]


def test_select_captured_launch_equals_eager_launches():
    W, G, L, n = 4, 3, 6, 5
    S = W * G
    x = (torch.randn(S, 512, generator=torch.Generator().manual_seed(9)) * 3).bfloat16().to(DEV)
    o = ops()
    allow, stop = o.pack_allow_mask(acgt_mask(), DEV), o.pack_allow_mask(stop_mask(), DEV)

    def state():
        cum = torch.full((S,), NEG, device=DEV)
        cum[::W] = 0.0
        return dict(cum=cum, ended=torch.zeros(S, dtype=torch.uint8, device=DEV), length=torch.zeros(S, dtype=torch.int64, device=DEV),
                    ids=torch.zeros(S, dtype=torch.int64, device=DEV), parent=torch.zeros(S, dtype=torch.int64, device=DEV),
                    hp=torch.full((S, L), -1, dtype=torch.int32, device=DEV), hi=torch.full((S, L), -1, dtype=torch.int64, device=DEV),
                    hc=torch.zeros(S, L, device=DEV), step=torch.zeros(G, dtype=torch.int64, device=DEV))

    def go(s):
        o.beam_select(x, s["cum"], s["ended"], s["length"], s["ids"], s["parent"], W, allow=allow, stop_mask=stop, hist_parent=s["hp"],
                      hist_ids=s["hi"], hist_cum=s["hc"], step=s["step"])
    a = state()
    go(a)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        go(a)
    for _ in range(n - 1):
        g.replay()
    torch.cuda.synchronize()
    b = state()
    for _ in range(n):
        go(b)
    torch.cuda.synchronize()
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert (a["step"] == n).all() and (a["hp"][:, :n] >= 0).all() and (a["hp"][:, n:] == -1).all()


# ------------------------------------------------------------------------------------------------ the reparenting copy
MAPS = {"identity": [0, 1, 2, 3, 4, 5], "one": [2, 2, 2, 2, 2, 2], "swap": [1, 0, 2, 3, 5, 4], "shift": [1, 2, 3, 4, 5, 0],
        "mixed": [0, 0, 3, 3, 5, 1], "clamped": [-7, 1, 99, 3, 4, 2 ** 40]}


def _bytes(shape, seed):
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("name", sorted(MAPS))
def test_gather_rows_equals_index_select(name):
    S, n_tok = 6, 7
    parent = torch.tensor(MAPS[name], dtype=torch.int64)
    p = parent.clamp(0, S - 1)
    own_pos = torch.tensor([-1, 0, 2, 6, 40, 3], dtype=torch.int64)    # live lengths 0, 1, partial, full, beyond the row (clamped), partial
    # fixed rows of 16, 3,072 (bf16 [S, 768, 2]) and 36,880 bytes (an odd number of 16-byte vectors, more than one workgroup's pass), a
    # complex64 tensor, and two per-token tensors [S, 7, ...] of 512 and 48 bytes per token; each sits inside a larger random buffer
    specs = [((S, 16), torch.uint8, False), ((S, 768, 2), torch.bfloat16, False), ((S, 36880), torch.uint8, False),
             ((S, 32, 8), torch.complex64, False), ((S, n_tok, 2, 1, 128), torch.bfloat16, True), ((S, n_tok, 48), torch.uint8, True)]
    bufs, views, want = [], [], []
    for k, (shape, dt, tok) in enumerate(specs):
        nbytes = int(torch.tensor(shape).prod()) * torch.empty((), dtype=dt).element_size()
        buf = _bytes((nbytes + 64,), 100 + k).to(DEV)
        v = buf[32:32 + nbytes].view(dt).view(shape)
        ref = buf.cpu().clone()
        rv = ref[32:32 + nbytes].view(S, -1)
        old = rv.clone()
        for s in range(S):
            if int(p[s]) != s:
                n = old.shape[1] if not tok else min(max(int(own_pos[p[s]]) + 1, 0), n_tok) * (old.shape[1] // n_tok)
                rv[s, :n] = old[p[s], :n]
        bufs.append(buf), views.append(v), want.append(ref)
    o = ops()
    tab = o.gather_table([v for v, s in zip(views, specs) if not s[2]], [v for v, s in zip(views, specs) if s[2]])
    assert tab.row_bytes == sum(w[32:-32].numel() // S for w in want) and tab.scratch_bytes == S * tab.row_bytes
    o.gather_rows(tab, parent.to(DEV), own_pos.to(DEV))
    torch.cuda.synchronize()
    for k, (buf, ref) in enumerate(zip(bufs, want)):
        assert torch.equal(buf.cpu(), ref), (name, k)                 # the rows, the bytes beyond the live lengths, the bytes around the tensor
    if name == "identity":
        assert all(torch.equal(b.cpu(), _bytes((b.numel(),), 100 + k)) for k, b in enumerate(bufs))


def test_gather_rows_in_a_graph_and_what_the_binding_refuses():
    S = 4
    a = torch.arange(S * 64, dtype=torch.float32, device=DEV).view(S, 64)
    o = ops()
    tab = o.gather_table([a])
    parent, own = torch.tensor([1, 2, 3, 0], device=DEV), torch.zeros(S, dtype=torch.int64, device=DEV)
    o.gather_rows(tab, parent, own)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        o.gather_rows(tab, parent, own)
    g.replay()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(a.cpu(), torch.arange(S * 64, dtype=torch.float32).view(S, 64).roll(-3, 0))      # three cyclic shifts
    with pytest.raises(RuntimeError):
        o.gather_table([torch.zeros(S, 3, device=DEV)])               # rows of 12 bytes
    with pytest.raises(RuntimeError):
        o.gather_table([a, torch.zeros(S + 1, 64, device=DEV)])
    with pytest.raises(RuntimeError):
        o.gather_rows(tab, parent[:3], own)


# ------------------------------------------------------------------------------------------------ arena
# `covers()` registers the entry points at IMPORT time: in a whole-suite run this module is what names the two entries for
# tests/test_gpu_arena.py's test_every_entry_point_is_named_by_a_case (as tests/test_gpu_stop.py does for its entry).
@covers("evo_beam_select_f32")
@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("hist", [True, False], ids=["history", "bare"])
def test_beam_select_in_the_arena(hist, f32):
    """W = 3, G = 2 and a leftover slot inside a poisoned arena: group 0 searches (a live, an ended and an empty beam), group 1 is
    inactive -- nothing of it but `parent` may change.  Rows of 520 elements (ld > V); per-slot vectors at their element's alignment."""
    o, g = ops(), gen(7)
    W, S, L = 3, 7, 4
    inp = {"lg": rnd((S, 520), g, 3.0, torch.float32 if f32 else torch.bfloat16),
           "cum": torch.tensor([-1.0, -0.5, NEG, -2.0, -3.0, -4.0, -5.0], device=DEV),
           "ended": torch.tensor([0, 1, 0, 0, 0, 0, 0], dtype=torch.uint8, device=DEV),
           "length": torch.arange(S, dtype=torch.int64, device=DEV) + 2, "ids": torch.arange(S, dtype=torch.int64, device=DEV) + 60,
           "active": torch.tensor([1, 0], dtype=torch.uint8, device=DEV), "allow": o.pack_allow_mask(acgt_mask(), DEV),
           "stop": o.pack_allow_mask(stop_mask(), DEV), "parent": poisoned((S,), torch.int64)}
    if hist:
        inp.update(hp=poisoned((S, L), torch.int32), hi=poisoned((S, L), torch.int64), hc=poisoned((S, L), torch.float32),
                   step=torch.tensor([2, 1], dtype=torch.int64, device=DEV))

    def fn(lg, cum, ended, length, ids, active, allow, stop, parent, hp=None, hi=None, hc=None, step=None):
        o.beam_select(lg[:, :512], cum, ended, length, ids, parent, W, group_active=active, allow=allow, stop_mask=stop, hist_parent=hp,
                      hist_ids=hi, hist_cum=hc, step=step)
    run = _run(fn, inp, inout=["cum", "ended", "length", "ids", "parent"] + (["hp", "hi", "hc", "step"] if hist else []),
               expect=["evo_beam_select_f32"],
               align={"cum": 4, "ended": 1, "length": 8, "ids": 8, "active": 1, "allow": 1, "stop": 1, "parent": 8, "hp": 4, "hi": 8, "hc": 4,
                      "step": 8})
    got = run.inputs
    assert got["parent"].tolist()[3:] == [3, 4, 5, 6] and set(got["parent"].tolist()[:3]) <= {0, 1}
    assert got["cum"].tolist()[3:] == [-2.0, -3.0, -4.0, -5.0] and got["ids"].tolist()[3:] == [63, 64, 65, 66]
    assert got["length"].tolist()[3:] == [5, 6, 7, 8] and -0.5 in got["cum"].tolist()[:3]          # the ended beam is carried
    if hist:
        assert got["step"].tolist() == [3, 1]
        assert is_poison(got["hp"][3:]) and is_poison(got["hp"][:3, :2]) and is_poison(got["hp"][:3, 3:]) and is_poison(got["hi"][3:])
        assert got["hp"][:3, 2].tolist() == got["parent"].tolist()[:3] and got["hi"][:3, 2].tolist() == got["ids"].tolist()[:3]
        assert torch.equal(got["hc"][:3, 2], got["cum"][:3]) and is_poison(got["hc"][3:])


@covers("evo_gather_rows")
@pytest.mark.parametrize("name", ["shift", "mixed", "clamped"])
def test_gather_rows_in_the_arena(name):
    """The table, the scratch buffer and both launches inside a poisoned arena: three tensors (fixed rows of 3,072 and 2,048 bytes, a
    per-token tensor of 512 bytes per token); the scratch buffer is allocated by the binding, i.e. carved from the arena too."""
    o, g = ops(), gen(11)
    S, n_tok = 6, 7
    inp = {"fir": rnd((S, 768, 2), g), "st": rnd((S, 32, 16), g, 1.0, torch.float32), "kv": rnd((S, n_tok, 2, 1, 128), g),
           "parent": torch.tensor(MAPS[name], dtype=torch.int64, device=DEV),
           "own_pos": torch.tensor([-1, 0, 2, 6, 40, 3], dtype=torch.int64, device=DEV)}
    want = {k: inp[k].clone() for k in ("fir", "st", "kv")}
    p = inp["parent"].clamp(0, S - 1).tolist()
    for s in range(S):
        if p[s] != s:
            n = min(max(int(inp["own_pos"][p[s]]) + 1, 0), n_tok)
            want["fir"][s], want["st"][s] = inp["fir"][p[s]], inp["st"][p[s]]
            want["kv"][s, :n] = inp["kv"][p[s], :n]

    def fn(fir, st, kv, parent, own_pos):
        o.gather_rows(o.gather_table([fir, st], [kv]), parent, own_pos)
    run = _run(fn, inp, inout=["fir", "st", "kv"], expect=["evo_gather_rows"], align={"parent": 8, "own_pos": 8})
    for k, w in want.items():
        assert torch.equal(run.inputs[k], w), (name, k)


# ------------------------------------------------------------------------------------------------ the pool
N_TOK, WEIGHTS_SEED = 12, 2                                           # (tests/test_gpu_stop.py: the weights of seed 2 leave some variety)
THREE = [PROMPTS[0], PROMPTS[1], PROMPTS[3]]                          # 81, 8 and 1 tokens: one shorter than the FIR history
_CACHE = {}


def toy():
    if "model" not in _CACHE:
        from evo_amd.tokenizer import CharLevelTokenizer
        cfgd = dict(SMALL4, use_interpolated_rotary_pos_emb=True, rotary_emb_scaling_factor=16)
        _CACHE["model"] = (build(cfgd, seed=WEIGHTS_SEED)[2], CharLevelTokenizer(512))
    return _CACHE["model"]


def beam_run(W, n_slots, use_graph, **kw):
    from evo_amd.pool import DecodePool
    key = (W, n_slots, use_graph, tuple(sorted(kw.items())))
    if key not in _CACHE:
        m, tok = toy()
        ctor = {k: kw[k] for k in ("weight_dtype",) if k in kw}
        pool = DecodePool(m, tok, n_slots=n_slots, device=DEV, use_graph=use_graph, allowed_tokens="ACGT", share_prompt_kv=True, **ctor)
        _CACHE[key] = (pool, pool.beam_search(THREE, N_TOK, beam_width=W, **{k: v for k, v in kw.items() if k not in ctor}))
    return _CACHE[key]


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_width_one_is_the_greedy_pool(use_graph):
    from evo_amd.pool import DecodePool
    m, tok = toy()
    pool, res = beam_run(1, 4, use_graph)
    greedy = DecodePool(m, tok, n_slots=4, top_k=1, device=DEV, use_graph=use_graph, seed=0, allowed_tokens="ACGT", share_prompt_kv=True)
    seqs, _, _ = greedy.generate(THREE, n_tokens=N_TOK)
    for j, r in enumerate(res):
        assert len(r) == 1 and r.lengths == [N_TOK]
        assert torch.equal(torch.tensor(list(r.sequences[0].encode())), greedy.last_ids[j]), j
    assert [r.sequences[0] for r in res] == seqs
    assert pool.stats["beam_rows_moved"] == 0 and pool.stats["beam_groups"] == 3


@pytest.mark.parametrize("use_graph", [True, False], ids=["graph", "eager"])
def test_forced_replay_reproduces_every_score_bit_for_bit(use_graph):
    import evo_amd
    from evo_amd.pool import DecodePool
    m, tok = toy()
    pool, res = beam_run(4, 8, use_graph)
    assert pool.stats["beam_rows_moved"] > 0 and pool.stats["beam_scratch_bytes"] == pool._beam["table"].scratch_bytes > 0
    assert (pool._beam_graph is not None) == use_graph
    hyps = [(pi, seq, score) for pi, r in enumerate(res) for seq, score in zip(r.sequences, r.scores)]
    assert len(hyps) == 12 and all(len(seq) == N_TOK for _, seq, _ in hyps)
    for r in res:
        assert r.scores == sorted(r.scores, reverse=True) and len(set(r.sequences)) == 4
        assert r.mean_scores == [s / n for s, n in zip(r.scores, r.lengths)]
    forced = DecodePool(m, tok, n_slots=8, device=DEV, use_graph=use_graph, allowed_tokens="ACGT", share_prompt_kv=True)
    seqs, _, _ = forced.generate([THREE[pi] for pi, _, _ in hyps], n_tokens=N_TOK,
                                 constraints=[evo_amd.iupac_template(seq) for _, seq, _ in hyps])
    assert seqs == [seq for _, seq, _ in hyps]
    bad = []
    for j, (pi, seq, score) in enumerate(hyps):
        cum = torch.zeros((), dtype=torch.float32)
        for lp in forced.last_logprobs[j, :N_TOK]:
            cum = cum + lp                                            # f32, in step order
        if float(cum) != score:
            bad.append((j, pi, seq, float(cum), score))
    print(f"[beam replay graph={use_graph}] {len(hyps)} hypotheses, rows moved {pool.stats['beam_rows_moved']}, mismatches {bad}")
    assert not bad, bad


def test_graph_and_eager_searches_agree():
    a, b = beam_run(4, 8, True)[1], beam_run(4, 8, False)[1]
    assert [(r.sequences, r.scores, r.lengths) for r in a] == [(r.sequences, r.scores, r.lengths) for r in b]


def test_every_recorded_choice_is_the_specifications():
    """Eager steps with the launch wrapped: every selection's inputs are recorded and the specification, on those logits and that state,
    must give what the step recorded: parent, token, ended and length exactly; cum within 2^-15 -- cum, logit and log-sum-exp stay
    below 64 in magnitude (asserted), where an f32 ulp is 2^-17 at most: three roundings and the kernel's own log-sum-exp.  A step
    whose best W + 1 candidates hold a near-tie of the model's own (the input condition of the kernel test) could be ranked either way
    by f32 and fp64; the weights and prompts are chosen so that there is none, and that is asserted: every step is compared."""
    from evo_amd.pool import DecodePool
    m, tok = toy()
    pool = DecodePool(m, tok, n_slots=8, device=DEV, use_graph=False, allowed_tokens="ACGT", share_prompt_kv=True)
    log, inner = [], pool._beam_select

    def recording(logits, group_active):
        b = pool._beam
        before = (logits.float().cpu(), b["cum"].cpu(), b["ended"].cpu(), b["length"].cpu(), pool.ids.view(-1).cpu(), group_active.cpu())
        inner(logits, group_active)
        log.append(before + (b["parent"].cpu(), pool.ids.view(-1).cpu(), b["cum"].cpu(), b["ended"].cpu(), b["length"].cpu()))
    pool._beam_select = recording
    res = pool.beam_search(THREE, 6, beam_width=4, stop_tokens="T", return_steps=True)
    assert len(log) == pool.stats["beam_steps"] + 3
    mask, stop = acgt_mask(), H.allowed_mask(tok, "T")
    skipped = 0
    for x, cum, ended, length, ids, active, p1, i1, c1, e1, n1 in log:
        if not condition_holds(x, cum, ended, ids, active, 4, mask):
            skipped += 1
            continue
        assert float(x[:, [ord(ch) for ch in "ACGT"]].abs().max()) < 64 and float(torch.logsumexp(x.double(), -1).abs().max()) < 64
        p, i, c, e, n = H.beam_select(x, cum, ended, length, ids, 4, active, mask, stop, dtype=torch.float64)
        rows = torch.cat([torch.arange(q * 4, q * 4 + 4) for q in range(2) if active[q]])
        assert torch.equal(p1[rows], p[rows]) and torch.equal(i1[rows], i[rows]) and torch.equal(e1[rows].bool(), e[rows])
        assert torch.equal(n1[rows], n[rows]) and torch.equal(torch.isinf(c1[rows]), torch.isinf(c[rows]))
        fin = ~torch.isinf(c[rows])
        assert float(c[rows][fin].abs().max()) < 64 and bool(((c1[rows][fin].double() - c[rows][fin]).abs() <= 2.0 ** -15).all())
    print(f"[beam steps] {len(log)} selections, {skipped} with a near-tie left out")
    assert skipped == 0                                               # (chosen so: with these weights and prompts no step holds a near-tie)
    for r in res:
        hp, hi, hc = r.steps
        assert hp.shape == hi.shape == hc.shape and hp.shape[0] == 4 and 1 <= hp.shape[1] <= 6
        assert [float(v) for v in hc[:len(r), -1]] == r.scores
        assert all("T" not in s for s in r.sequences)


def test_fp8_weights_compose():
    pool, res = beam_run(4, 8, True, weight_dtype="fp8")
    assert pool.stats["weight_dtype"] == "fp8" and len(res) == 3
    for r in res:
        assert len(r) == 4 and r.scores == sorted(r.scores, reverse=True) and all(set(s) <= set("ACGT") and len(s) == N_TOK for s in r.sequences)
    assert [r.sequences for r in res] != [r.sequences for r in beam_run(4, 8, True)[1]] or \
        [r.scores for r in res] != [r.scores for r in beam_run(4, 8, True)[1]]          # the FP8 step really ran
