"""CPU: the written specification of the device sampler (evo_amd/sh/sample.py: Philox4x32-10, seeded_uniform, sample_seeded,
allowed_mask) and the host-side argument checks of evo_sample_rows_f32, which need no GPU."""
import ctypes

import numpy as np
import pytest
import torch

from evo_amd.sh import sample as S
from evo_amd.tokenizer import CharLevelTokenizer


def _hex(words):
    return " ".join("%08x" % int(w) for w in words)


def test_philox_known_answers():
    assert _hex(S.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert _hex(S.philox4x32_10((ones,) * 4, (ones,) * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(S.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) \
        == "d16cfe09 94fdcceb 5001e420 24126ea1"
    # the array form is the scalar form, element by element
    c = [np.array([0, ones, 0x243F6A88], dtype=np.uint64), np.array([0, ones, 0x85A308D3], dtype=np.uint64),
         np.array([0, ones, 0x13198A2E], dtype=np.uint64), np.array([0, ones, 0x03707344], dtype=np.uint64)]
    k = [np.array([0, ones, 0xA4093822], dtype=np.uint64), np.array([0, ones, 0x299F31D0], dtype=np.uint64)]
    out = S.philox4x32_10(c, k)
    assert _hex(w[2] for w in out) == "d16cfe09 94fdcceb 5001e420 24126ea1" and _hex(w[0] for w in out).startswith("6627e8d5")


def test_seeded_uniform_is_a_function_of_seed_stream_count():
    u = S.seeded_uniform(7, 3, 5)
    assert 0.0 < u < 1.0 and u == S.seeded_uniform(7, 3, 5)
    assert len({u, S.seeded_uniform(8, 3, 5), S.seeded_uniform(7, 4, 5), S.seeded_uniform(7, 3, 6)}) == 4
    many = S.seeded_uniform(7, np.arange(4096), 5)
    assert many.shape == (4096,) and (many > 0).all() and (many < 1).all() and many[3] == u
    assert S.seeded_uniform(7, 3, np.array([5, 6]))[1] == S.seeded_uniform(7, 3, 6)
    assert S.seeded_uniform(2 ** 40 + 7, 2 ** 33 + 1, 2 ** 35) != S.seeded_uniform(7, 1, 0)      # the high words count
    assert 0.3 < many.mean() < 0.7


@pytest.mark.parametrize("top_k,top_p,temperature", [(50, 0.7, 1.0), (4, 0.9, 0.7), (0, 0.95, 1.2), (4, 1.0, 0.7), (0, 1.0, 1.0)])
def test_sample_seeded_keeps_the_tokens_the_filters_keep(top_k, top_p, temperature):
    g = torch.Generator().manual_seed(11)
    row = torch.randn(1, 512, generator=g) * (1.0 if top_k == 0 else 3.0)        # (no ties: the filters' own set is well defined)
    ref = row.clone().float()
    if top_k > 0:
        S.modify_logits_for_top_k_filtering(ref, min(top_k, 512))
    if temperature != 1.0 and temperature > 0.0:
        ref /= temperature
    S.modify_logits_for_top_p_filtering(ref, top_p)
    kept = set(torch.nonzero(ref[0] > float("-inf")).flatten().tolist())
    n = 10 ** 4
    toks = S.sample_seeded(row.expand(n, 512), top_k, top_p, temperature, seed=5, stream=np.arange(n), count=0)
    support = set(toks.tolist())
    assert support <= kept
    if len(kept) <= 50:                                               # every kept token this likely shows up in 10^4 draws
        p = torch.softmax(ref[0].double(), -1)
        likely = {t for t in kept if p[t] * n > 25}
        assert likely <= support, (sorted(likely - support))
    order, cdf, n_kept = S.seeded_distribution(row, top_k, top_p, temperature)
    assert set(order[0, : int(n_kept[0])].tolist()) == kept


def test_top_p_cut_inside_a_tie_keeps_the_filters_count_and_the_lowest_ids():
    row = torch.full((1, 512), -30.0)
    row[0, [10, 20, 30, 40]] = 2.0                                    # four equal tokens of probability ~ 1/4 each
    ref = row.clone().double()
    S.modify_logits_for_top_p_filtering(ref, 0.6)                     # drops while cum <= 0.4: one of the four goes
    assert int((ref[0] > float("-inf")).sum()) == 3
    order, cdf, n_kept = S.seeded_distribution(row, 0, 0.6, 1.0)
    assert int(n_kept[0]) == 3 and order[0, :3].tolist() == [10, 20, 30]
    toks = S.sample_seeded(row.expand(500, 512), 0, 0.6, 1.0, seed=1, stream=np.arange(500), count=0)
    assert set(toks.tolist()) == {10, 20, 30}


def test_top_k_1_is_argmax_lowest_id_on_ties():
    g = torch.Generator().manual_seed(3)
    rows = (torch.randn(64, 512, generator=g) * 3).bfloat16().float()
    toks = S.sample_seeded(rows, 1, 0.7, 0.5, seed=9, stream=np.arange(64), count=4)
    assert torch.equal(toks, rows.argmax(-1))
    rows[:, 100] = rows[:, 7] = rows.max() + 1
    assert S.sample_seeded(rows, 1, 1.0, 1.0, seed=9, stream=0, count=0).tolist() == [7] * 64
    assert int(S.sample_seeded(rows[0], 1, 1.0, 1.0, seed=9, stream=0, count=0)) == 7


def test_allowed_mask():
    tok = CharLevelTokenizer(512)
    m = S.allowed_mask(tok, "ACGT")
    assert m.dtype == torch.bool and m.shape == (512,) and torch.nonzero(m).flatten().tolist() == [65, 67, 71, 84]
    assert torch.equal(S.allowed_mask(tok, [84, 71, 67, 65, 65]), m)
    g = torch.Generator().manual_seed(0)
    rows = torch.randn(2000, 512, generator=g) * 3
    for top_k, top_p, t in ((50, 0.7, 1.0), (0, 1.0, 1.0), (1, 1.0, 1.0), (2, 0.9, 0.7)):
        toks = S.sample_seeded(rows, top_k, top_p, t, seed=3, stream=np.arange(2000), count=1, allowed=m)
        assert set(toks.tolist()) <= {65, 67, 71, 84}
    for bad in ("", [], [512], [-1], [3, 700]):
        with pytest.raises(ValueError):
            S.allowed_mask(tok, bad)


def test_existing_sampler_is_untouched_by_the_additions():
    torch.manual_seed(0)
    x = torch.randn(8, 512)
    assert torch.equal(S.sample(x, top_k=1), x.argmax(-1))
    torch.manual_seed(1)
    a = S.sample(x, top_k=4, top_p=1.0, temperature=0.7)
    torch.manual_seed(1)
    assert torch.equal(a, S.sample(x, top_k=4, top_p=1.0, temperature=0.7))


def test_sample_rows_argument_validation_needs_no_gpu():
    from evo_amd import ops as evo_ops
    lib = evo_ops.load_library()
    f = lib.evo_sample_rows_f32
    one = ctypes.c_void_p(16)                                         # (non-null, 16-byte aligned, never dereferenced)
    # (logits, logits_f32, ld, top_k, top_p, temperature, allow, seed, stream, count, active, ids_out, logprob_out,
    #  hist_ids, hist_logits, hist_len, S, V, hip stream)
    ok = [one, 0, 512, one, one, one, None, 1, None, None, None, one, one, None, None, 0, 4, 512, None]

    def call(**kw):
        a = list(ok)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return f(*a)
    assert call(a16=0) == -1                                          # S < 1
    assert call(a17=256) == -1                                        # V must be 512
    assert call(a0=None) == -1 and call(a11=None) == -1 and call(a12=None) == -1      # null logits / outputs
    assert call(a3=None) == -1 and call(a4=None) == -1 and call(a5=None) == -1        # null per-row settings
    assert call(a2=500) == -1 and call(a2=516) == -1                  # row pitch below V / not a multiple of 8
    assert call(a0=ctypes.c_void_p(8)) == -1                          # logits not 16-byte aligned
    assert call(a13=one, a15=8) == -1 and call(a14=one, a15=8) == -1  # history without count
    assert call(a13=one, a9=one, a15=0) == -1                         # history without room
    assert evo_ops.ABI_VERSION >= 12
