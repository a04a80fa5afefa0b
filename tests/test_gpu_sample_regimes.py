"""GPU (-m gpu): the device sampler (csrc/sample.hip, HipOps.sample_rows) where tests/test_gpu_sample.py cannot see it.

1. FLAT rows (tests/select_ref.py; pinned to the specification by tests/test_select_ref_host.py): temperature 2^40 makes every kept
   token's weight exactly 1.0f, so the token is order[floor(u n)] and is compared for EQUALITY -- the whole sorted order, the tie rule
   at every position, the k-th value's ties, -inf entries, masks that leave 1 / 4 / 509 tokens, top_k from -1 to 2^31 - 1 and the top-p
   cut, with top_k / top_p / temperature differing from row to row inside one launch.  A row is left out only when u n lies within
   2^-12 of an integer (at most 0.5 % of a launch).
2. 64-bit keying: seeds, stream ids and counts whose high words are not 0, each against the same launch with that value truncated to
   32 bits.
3. Non-flat extremes (temperature 0.05 / 30 / 0 / -1, f32 rows over +-3e4, a +60 spike, the two largest logits equal) under
   test_gpu_sample.py's own acceptance rule (d = 2^-14, at most 4 % of a setting undecidable), and logprob_out against fp64."""
import numpy as np
import pytest
import torch

import rowlocal_ref as RL
import select_ref as SR
from test_gpu_sample import accept

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def ops():
    from evo_amd.ops import default_ops
    return default_ops()


def dev(t):
    return t.to(DEV).contiguous()


def launch(rows, c, sl, seed, allow=None, stream=None, count=None, **kw):
    """One launch on the rows `sl` of the flat case `c`; returns (ids on the host, the advanced count on the host)."""
    cnt = dev(c["count"][sl] if count is None else count)
    ids, lp = ops().sample_rows(rows, dev(c["top_k"][sl]), dev(c["top_p"][sl]), dev(c["temperature"][sl]), seed,
                                stream=dev(c["stream"][sl] if stream is None else stream), count=cnt, allow=allow, **kw)
    torch.cuda.synchronize()
    return ids.cpu(), cnt.cpu()


def mismatches(ids, tok, out):
    bad = (ids != tok) & ~out
    return int(bad.sum()), torch.nonzero(bad).flatten()[:8].tolist()


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("mask_name", SR.MASKS)
def test_flat_rows_exact_tokens_heterogeneous_launch(mask_name, f32):
    c = SR.flat_case()
    S = c["rows"].shape[0]
    tok, out, n, _ = SR.flat_expected(mask_name)
    share = out.float().mean().item()
    assert share <= SR.U_CAP, share
    mask = SR.flat_mask(mask_name)
    allow = ops().pack_allow_mask(mask, DEV) if mask is not None else None
    rows = dev(c["rows"] if f32 else c["rows"].bfloat16())
    ids, cnt = launch(rows, c, slice(None), SR.FLAT_SEED, allow)
    assert torch.equal(cnt, c["count"] + 1)                               # exactly one per row
    nbad, first = mismatches(ids, tok, out)
    print(f"[sample regimes flat mask={mask_name} f32={f32}] rows left out {100 * share:.3f} %, mismatches {nbad} of {S}")
    assert nbad == 0, (nbad, first, [(int(c['kind'][r]), int(c['top_k'][r]), float(c['top_p'][r]), int(n[r])) for r in first])
    for s in (1, 5, 33):                                                  # a row's token does not depend on the rows around it
        part, cnt = launch(rows[:s], c, slice(0, s), SR.FLAT_SEED, allow)
        assert torch.equal(part, ids[:s]) and torch.equal(cnt, c["count"][:s] + 1), s
    # a row pitch of 1024: the left half of a [S, 1024] matrix, which sample_rows takes as it is (no copy)
    wide = torch.full((S, 1024), 7.0, dtype=rows.dtype, device=DEV)
    wide[:, :512] = rows
    view = wide[:, :512]
    assert view.stride(0) == 1024 and not view.is_contiguous()
    pitched, _ = launch(view, c, slice(None), SR.FLAT_SEED, allow)
    assert torch.equal(pitched, ids)


def test_flat_rows_past_65535_workgroups():
    c = SR.flat_case()
    S, base = 70000, c["rows"].shape[0]
    _, _, n, od = SR.flat_expected("none")
    r = torch.arange(S) % base
    big = {k: v[r] for k, v in c.items() if k != "rows"}
    big["stream"] = torch.arange(S, dtype=torch.int64) * 3 + 2
    big["count"] = (torch.arange(S, dtype=torch.int64) * 7) % 1000
    tok, out = SR.flat_draw(od[0], n, c["top_k"], SR.FLAT_SEED + 1, big["stream"].numpy(), big["count"].numpy(), index=r)
    share = out.float().mean().item()
    assert share <= SR.U_CAP, share
    for f32 in (False, True):
        rows = dev(c["rows"] if f32 else c["rows"].bfloat16())[r.to(DEV)]
        ids, cnt = launch(rows, big, slice(None), SR.FLAT_SEED + 1)
        nbad, first = mismatches(ids, tok, out)
        print(f"[sample regimes flat S={S} f32={f32}] rows left out {100 * share:.3f} %, mismatches {nbad}")
        assert nbad == 0, (nbad, first)
        assert torch.equal(cnt, big["count"] + 1)
        del rows


def keying_case():
    """2,048 rows of the flat case that keep all 512 tokens (no -inf entry), with top_k = 0 and top_p = 1: the token identifies
    floor(512 u) wherever the row's values differ."""
    c = SR.flat_case()
    idx = torch.nonzero(c["kind"] < 12).flatten()[:2048]
    S = idx.numel()
    kc = dict(rows=c["rows"][idx], top_k=torch.zeros(S, dtype=torch.int32), top_p=torch.ones(S), temperature=torch.full((S,), SR.FLAT_T))
    return kc, SR.flat_order(kc["rows"])


def test_keying_uses_all_64_bits_of_seed_stream_and_count():
    kc, od = keying_case()
    S = kc["rows"].shape[0]
    assert int(od[1].min()) == 512
    rows = dev(kc["rows"].bfloat16())
    j = np.arange(S, dtype=np.int64)

    def run(seed, st, ct):
        st, ct = torch.from_numpy(np.asarray(st, dtype=np.int64)), torch.from_numpy(np.asarray(ct, dtype=np.int64))
        ids, cnt = launch(rows, kc, slice(None), seed, stream=st, count=ct)
        assert torch.equal(cnt, ct + 1)
        return ids

    worst = 0.0
    for seed in SR.SEEDS64:
        for sname, sf in SR.STREAMS64.items():
            for cname, cf in SR.COUNTS64.items():
                st, ct = np.asarray(sf(j), dtype=np.int64), np.asarray(cf(j), dtype=np.int64)
                tok, out, _ = SR.flat_predict(None, kc["top_k"], kc["top_p"], None, seed, st, ct, order=od)
                share = out.float().mean().item()
                worst = max(worst, share)
                assert share <= SR.U_CAP, (seed, sname, cname, share)
                ids = run(seed, st, ct)
                nbad, first = mismatches(ids, tok, out)
                assert nbad == 0, (seed, sname, cname, nbad, first)
                # the same launch with ONE value truncated to its low word draws other tokens: the test sees the high words
                if seed != SR.low32(seed) and sname == "j" and cname == "j":
                    assert (run(SR.low32(seed), st, ct) != ids).float().mean().item() > 0.2, seed
                if seed == 5 and sname != "j" and cname == "j":
                    assert (run(seed, SR.low32(st), ct) != ids).float().mean().item() > 0.2, sname
                if seed == 5 and sname == "j" and cname != "j":
                    assert (run(seed, st, SR.low32(ct)) != ids).float().mean().item() > 0.2, cname
    print(f"[sample regimes keying] 48 launches of {S} rows, largest share left out {100 * worst:.3f} %, mismatches 0")


def test_history_records_nothing_at_count_2_pow_32():
    kc, od = keying_case()
    S, L = 64, 4
    rows = dev(kc["rows"][:S].bfloat16())
    sub = {k: v[:S] for k, v in kc.items()}
    count0 = torch.where(torch.arange(S) % 2 == 0, torch.tensor(2 ** 32), torch.tensor(2))      # low word 0 would land in slot 0
    count0[5] = 2 ** 32 + 1
    hid = torch.full((S, L), -9, dtype=torch.int64, device=DEV)
    hlg = torch.full((S, L, 512), 777.0, dtype=torch.float32, device=DEV)
    st = torch.arange(S, dtype=torch.int64) + 100
    ids, cnt = launch(rows, sub, slice(None), 9, stream=st, count=count0, hist_ids=hid, hist_logits=hlg)
    assert torch.equal(cnt, count0 + 1)
    tok, out, _ = SR.flat_predict(None, sub["top_k"], sub["top_p"], None, 9, st.numpy(), count0.numpy(), order=tuple(t[:S] for t in od))
    assert mismatches(ids, tok, out)[0] == 0
    want_hid = torch.full((S, L), -9, dtype=torch.int64)
    want_hlg = torch.full((S, L, 512), 777.0)
    rec = torch.nonzero(count0 < L).flatten()
    want_hid[rec, 2] = ids[rec]
    want_hlg[rec, 2] = kc["rows"][rec]
    assert torch.equal(hid.cpu(), want_hid) and torch.equal(hlg.cpu(), want_hlg)


@pytest.mark.parametrize("name,f32,settings,logprob", SR.EXTREME_CASES, ids=[c[0] for c in SR.EXTREME_CASES])
def test_extreme_rows_under_the_acceptance_rule(name, f32, settings, logprob):
    rows = SR.extreme_rows(name)
    n = rows.shape[0]
    dev_rows = dev(rows)
    stream, count = SR.extreme_keys(n)
    for k, p, T in settings:
        tk = torch.full((n,), k, dtype=torch.int32, device=DEV)
        tp = torch.full((n,), p, dtype=torch.float32, device=DEV)
        tt = torch.full((n,), T, dtype=torch.float32, device=DEV)
        cnt = dev(torch.from_numpy(count))
        ids, lp = ops().sample_rows(dev_rows, tk, tp, tt, SR.EXTREME_SEED, stream=dev(torch.from_numpy(stream)), count=cnt)
        torch.cuda.synchronize()
        ids, lp = ids.cpu(), lp.cpu()
        assert int(ids.min()) >= 0 and int(ids.max()) < 512
        out, bad = accept(rows, ids, k, p, T, None, SR.EXTREME_SEED, stream, count)
        share = out.float().mean().item()
        print(f"[sample regimes {name} k={k} p={p} T={T}] rows left out {100 * share:.2f} %, rejected {int(bad.sum())}, "
              f"distinct tokens {ids.unique().numel()}")
        assert share <= SR.UNDECIDABLE_CAP, share
        assert int(bad.sum()) == 0, torch.nonzero(bad).flatten()[:8].tolist()
        if logprob:
            r = torch.arange(n)
            ref = torch.log_softmax(rows.double(), -1)[r, ids]
            x = dev_rows.float()
            mx = x.max(-1, keepdim=True)[0]
            f32v = (x - (mx + (x - mx).exp().sum(-1, keepdim=True).log())).cpu()[r, ids]
            allow, e32 = RL.measured_allowance(ref, f32v)
            err = (lp.double() - ref).abs()
            print(f"[sample regimes {name} k={k} p={p} T={T}] logprob max |err| {float(err.max()):.3e}, fp32 torch restatement {e32:.3e}")
            assert bool((err <= allow).all()), (float(err.max()), e32)
