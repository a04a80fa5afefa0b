"""GPU (-m gpu): the profile epilogue of the fused scoring tail (evo_unembed_profile_bf16) and the API above it.

Kernel level: bit for bit against the shipped entry (evo_unembed_logprob_bf16 with target = the selected id: the kernel body is
shared, so the tolerance is zero -- a mismatch means the body diverged), against the fp64 oracle on bf16-rounded logits within the
bounds of test_gpu_kernels.test_fused_unembed_logprob_matches_two_kernel_path_and_oracle (max <= 2.5 ulp, mean <= 0.25 ulp, ulp =
max|logit| 2^-7), every one of the 512 columns once, and with the optional outputs switched off.  Model level: position_profiles on
the HIP engine equals, bit for bit, the per-token values behind score_sequences and positional_entropies.

The arena cases of the new entry live here too (tests/test_gpu_arena.py is not edited): `covers` registers the entry at import, so
test_gpu_arena.test_every_entry_point_is_named_by_a_case sees it whenever both modules are collected -- `pytest tests -m gpu`, the
documented way to run the suite.  Running test_gpu_arena.py ALONE names evo_unembed_profile_bf16 as uncovered."""
import math

import numpy as np
import pytest
import torch

from oracle import stripedhyena_ref as R
from test_gpu_arena import _run, covers, gen, rnd

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SHAPES = [(1, 32),                               # one row, one k-step
          (63, 64), (64, 32), (65, 288),         # around the 64-row tile edge, K % 256 != 0
          (130, 4096)]                           # three workgroups at the model's width
TOKEN_SETS = [[65, 67, 71, 84],
              [0],
              [511, 4, 260, 8, 131, 32, 384, 67]]    # unsorted; all four waves' column ranges, both lane halves, every column-index bit set in one id and clear in another


@pytest.fixture(scope="module")
def ops():
    from evo_amd.ops import HipOps
    return HipOps()


def _cpu_gen(seed):
    return torch.Generator().manual_seed(seed)


_CASES = {}


def case(M, K):
    """Inputs of the existing tail test (randn hidden, randn * 4 / sqrt(K) embedding), targets with a masked row, and the fp64
    log-softmax / entropy of the bf16-rounded logits -- computed once per shape, shared, never modified."""
    if (M, K) not in _CASES:
        hid = torch.randn(M, K, generator=_cpu_gen(30)).to(torch.bfloat16)
        emb = (torch.randn(512, K, generator=_cpu_gen(31)) * (4.0 / math.sqrt(K))).to(torch.bfloat16)
        tgt = torch.randint(0, 512, (M,), generator=_cpu_gen(32))
        tgt[M // 2] = -1                                                   # masked position -> log-prob 0
        logits = (hid.double() @ emb.double().t()).to(torch.bfloat16)      # one rounding of every logit to bf16
        rlp, ren = R.op_logprob_entropy(logits, tgt)
        lsm = torch.log_softmax(logits.double(), -1)
        ulp = float(logits.abs().max()) * 2 ** -7
        _CASES[(M, K)] = dict(hid=hid.to(DEV), emb=emb.to(DEV), tgt=tgt.to(DEV), rlp=rlp, ren=ren, lsm=lsm, ulp=ulp)
    return _CASES[(M, K)]


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("sel", TOKEN_SETS, ids=lambda s: "n%d" % len(s))
@pytest.mark.parametrize("M,K", SHAPES)
def test_profile_kernel_equals_the_shipped_entry_bitwise_and_the_oracle(ops, M, K, sel):
    c = case(M, K)
    sl, lp, en = ops.unembed_profile(c["hid"], c["emb"], sel, c["tgt"])
    assert sl.shape == (M, len(sel)) and sl.dtype == torch.float32 and lp.shape == (M,) and en.shape == (M,)
    # (a) the shipped entry: log-prob / entropy with the same targets, and target = sel[j] for every selected column
    lp0, en0 = ops.unembed_logprob(c["hid"], c["emb"], c["tgt"], want_logprob=True, want_entropy=True)
    assert same_bits(lp, lp0) and same_bits(en, en0)
    assert lp[M // 2].item() == 0.0
    for j, t in enumerate(sel):
        col, _ = ops.unembed_logprob(c["hid"], c["emb"], torch.full((M,), t, dtype=torch.int64, device=DEV))
        assert same_bits(sl[:, j], col), (j, t, (sl[:, j] - col).abs().max().item())
    # (b) the fp64 oracle on bf16-rounded logits
    err = (sl.double().cpu() - c["lsm"][:, sel]).abs()
    e_lp = (lp.double().cpu() - c["rlp"]).abs()
    e_en = (en.double().cpu() - c["ren"]).abs()
    print(f"M={M} K={K} n={len(sel)}: ulp {c['ulp']:.3e}  sel max {err.max() / c['ulp']:.3f} mean {err.mean() / c['ulp']:.4f} ulp  "
          f"logprob max {e_lp.max() / c['ulp']:.3f}  entropy max {e_en.max() / c['ulp']:.3f}")
    assert err.max() <= 2.5 * c["ulp"] and err.mean() <= 0.25 * c["ulp"]
    assert e_lp.max() <= 2.5 * c["ulp"] and e_lp.mean() <= 0.25 * c["ulp"]
    assert e_en.max() <= 2.5 * c["ulp"]
    # (c) the optional outputs off (NULL pointers): the selected columns are unchanged; no target at all: the same
    sl2, lp2, en2 = ops.unembed_profile(c["hid"], c["emb"], sel, c["tgt"], want_logprob=False, want_entropy=False)
    assert lp2 is None and en2 is None and same_bits(sl2, sl)
    sl3, lp3, en3 = ops.unembed_profile(c["hid"], c["emb"], sel, None)
    assert same_bits(sl3, sl) and same_bits(en3, en) and not lp3.any()


def test_every_column_is_mapped_once(ops):
    """(65, 64): a seeded permutation of the 512 ids cut into 64 sets of 8 -- the concatenated result is the whole log-softmax.  A
    mapping error would put another column's logit in place: whole units off (the logits' standard deviation is about 4)."""
    M, K = 65, 64
    c = case(M, K)
    perm = torch.randperm(512, generator=_cpu_gen(5)).tolist()
    got = torch.empty(M, 512, dtype=torch.float64)
    for s in range(0, 512, 8):
        ids = perm[s:s + 8]
        sl, _, _ = ops.unembed_profile(c["hid"], c["emb"], ids, None, want_logprob=False, want_entropy=False)
        got[:, ids] = sl.double().cpu()
    err = (got - c["lsm"]).abs()
    print(f"all 512 columns: max {err.max() / c['ulp']:.3f} ulp, mean {err.mean() / c['ulp']:.4f} ulp")
    assert err.max() <= 2.5 * c["ulp"]


def test_binding_refuses_bad_ids_and_operands(ops):
    c = case(1, 32)
    for bad in ([], list(range(9)), [7, 7], [512], [-1]):
        with pytest.raises(ValueError):
            ops.unembed_profile(c["hid"], c["emb"], bad)
    with pytest.raises(RuntimeError):
        ops.unembed_profile(c["hid"].float(), c["emb"], [65])
    with pytest.raises(RuntimeError):
        ops.unembed_profile(c["hid"].cpu(), c["emb"], [65])


# ------------------------------------------------------------------------------------------------ model level
LENGTHS = (5, 63, 64, 130)          # B * T crosses several 64-row tiles, the sequences end mid-tile


@pytest.fixture(scope="module")
def small_engine():
    from test_gpu_model import SMALL, build
    from evo_amd.tokenizer import CharLevelTokenizer
    cfg, sd, m = build(SMALL)
    rng = np.random.default_rng(21)
    seqs = ["".join(rng.choice(list("ACGT"), size=n)) for n in LENGTHS]
    return m, CharLevelTokenizer(512), seqs


def test_position_profiles_equal_the_scoring_paths_bitwise(small_engine, monkeypatch):
    import evo_amd
    from evo_amd.scoring import prepare_batch, score_logprobs_device
    m, tok, seqs = small_engine
    monkeypatch.delenv("EVO_AMD_FUSED_TAIL", raising=False)
    calls = []
    real = m.ops.unembed_profile
    monkeypatch.setattr(m.ops, "unembed_profile", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    profs = evo_amd.position_profiles(seqs, m, tok, device=DEV)
    assert calls == [1]                                                     # ONE launch of the profile entry, no logits
    ids, lens = prepare_batch(seqs, tok, device=DEV)
    with torch.inference_mode():
        lp, _ = score_logprobs_device(m, ids)                               # the per-token values behind score_sequences
    lp = lp.float().cpu().numpy()
    ents = evo_amd.positional_entropies(seqs, m, tok, device=DEV)
    sums = evo_amd.score_sequences(seqs, m, tok, reduce_method="sum", device=DEV)
    for i, (s, p) in enumerate(zip(seqs, profs)):
        assert p.tokens == (65, 67, 71, 84) and p.token_logprobs.shape == (len(s), 4)
        assert np.array_equal(p.logprob.view(np.int32), lp[i][:len(s)].view(np.int32))
        assert np.array_equal(p.entropy.view(np.int32), ents[i].view(np.int32))
        assert np.sum(p.logprob) == sums[i]
        sub = evo_amd.substitution_scores(p)
        for j, ch in enumerate("ACGT"):
            at = np.array([x == ch for x in s])
            assert np.array_equal(p.token_logprobs[at, j].view(np.int32), p.logprob[at].view(np.int32))
            assert (sub[at, j] == 0.0).all()
        assert np.isfinite(p.token_logprobs).all() and (p.token_logprobs < 0).all()

    # the fallback (model(ids) -> fp32 log-softmax) agrees within 2.5 ulp of this model's logits
    with torch.inference_mode():
        logits = m(ids)[0]
    ulp = float(logits.float().abs().max()) * 2 ** -7
    monkeypatch.setenv("EVO_AMD_FUSED_TAIL", "0")
    calls.clear()
    slow = evo_amd.position_profiles(seqs, m, tok, device=DEV)
    assert calls == []
    for p, q in zip(profs, slow):
        d = max(np.abs(p.token_logprobs - q.token_logprobs).max(), np.abs(p.logprob - q.logprob).max(), np.abs(p.entropy - q.entropy).max())
        print(f"L={len(p.logprob)}: fused vs fallback {d / ulp:.3f} ulp (ulp {ulp:.3e})")
        assert d <= 2.5 * ulp


# ------------------------------------------------------------------------------------------------ arena
@covers("evo_unembed_profile_bf16")
@pytest.mark.parametrize("n_sel", [1, 3, 8])                 # n_sel = 3: rows of sel_logprob of 12 bytes -- only the base is 16-byte aligned
@pytest.mark.parametrize("M,K", [(70, 32), (63, 4096), (513, 256)])
def test_unembed_profile_in_the_arena(M, K, n_sel):
    import evo_amd.ops as evo_ops
    ops, g = evo_ops.default_ops(), gen(30)
    tgt = torch.randint(0, 512, (M,), device=DEV, generator=g)
    tgt[M // 2] = -1
    sel = [511, 4, 260, 8, 131, 32, 384, 67][:n_sel]
    inp = {"hid": rnd((M, K), g), "emb": rnd((512, K), g, 4.0 / math.sqrt(K)), "tgt": tgt}
    assert ops.unembed_logprob_ok(inp["hid"], inp["emb"])
    _run(lambda hid, emb, tgt: ops.unembed_profile(hid, emb, sel, tgt, want_logprob=True, want_entropy=True), inp,
         expect=["evo_unembed_profile_bf16"], align={"tgt": 8})
