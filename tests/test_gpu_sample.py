"""GPU (-m gpu): the device sampler (csrc/sample.hip, HipOps.sample_rows) against its written specification
(evo_amd/sh/sample.py: sample_seeded, fp64 on the CPU).

Acceptance of a token.  The kernel's sums are fp32, the specification's fp64, so a draw whose u falls within
d = 2^-14 of a CDF boundary may go either way (d = twice the worst-case error 512 * 2^-24 of an fp32 prefix sum of 512 terms
that add up to 1, the factor 2 for the exponentials), and nothing else may: the token t, at position i of the order
"descending logit, ascending id", must be in the kept set and satisfy cdf64[i - 1] - d <= u < cdf64[i] + d.  A row is left out
only when its top-p cut is undecidable -- some fp64 cumulative value of the filter lies within d of 1 - top_p -- and the share
of such rows is capped at 4 % per setting.  top_k compares the input values themselves: no tolerance."""
import numpy as np
import pytest
import torch

from evo_amd.sh import sample as H
from evo_amd.tokenizer import CharLevelTokenizer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
D_TOL = 2.0 ** -14
SETTINGS = [(50, 0.7, 1.0, 3.0), (4, 0.9, 0.7, 3.0), (0, 0.95, 1.2, 6.0), (4, 1.0, 0.7, 3.0), (0, 1.0, 1.0, 3.0)]


def ops():
    from evo_amd.ops import default_ops
    return default_ops()


def rows_bf16(n, sigma, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(n, 512, generator=g) * sigma).bfloat16()


def params(S, top_k, top_p, temperature):
    return (torch.full((S,), top_k, dtype=torch.int32, device=DEV), torch.full((S,), top_p, dtype=torch.float32, device=DEV),
            torch.full((S,), temperature, dtype=torch.float32, device=DEV))


def acgt_mask():
    return H.allowed_mask(CharLevelTokenizer(512), "ACGT")


def undecidable(rows, top_k, top_p, temperature, mask):
    """Rows whose top-p cut an fp32 sum cannot decide: an fp64 cumulative value of the filter within D_TOL of 1 - top_p."""
    if not 0.0 < top_p < 1.0:
        return torch.zeros(rows.shape[0], dtype=torch.bool)
    x = rows.double().clone()
    if mask is not None:
        x.masked_fill_(~mask[None, :], float("-inf"))
    if top_k > 0:
        H.modify_logits_for_top_k_filtering(x, min(top_k, 512))
    if temperature != 1.0 and temperature > 0.0:
        x /= temperature
    cum = torch.sort(x, descending=False)[0].softmax(-1).cumsum(-1)
    return ((cum - (1.0 - top_p)).abs() <= D_TOL).any(-1)


def accept(rows, toks, top_k, top_p, temperature, mask, seed, stream, count):
    """(rows left out [n] bool, rows whose token the specification does not accept [n] bool)."""
    rows = rows.detach().cpu()
    toks = toks.detach().cpu()
    order, cdf, n_kept = H.seeded_distribution(rows, top_k, top_p, temperature, mask)
    out = undecidable(rows, top_k, top_p, temperature, mask)
    pos = torch.argsort(order, dim=-1).gather(-1, toks[:, None])[:, 0]
    u = torch.from_numpy(np.ascontiguousarray(H.seeded_uniform(seed, np.broadcast_to(np.asarray(stream), (rows.shape[0],)),
                                                                np.broadcast_to(np.asarray(count), (rows.shape[0],)))))
    hi = cdf.gather(-1, pos[:, None])[:, 0]
    lo = torch.where(pos > 0, cdf.gather(-1, (pos - 1).clamp(min=0)[:, None])[:, 0], torch.zeros_like(hi))
    good = (pos < n_kept) & (lo - D_TOL <= u) & (u < hi + D_TOL)
    return out, ~good & ~out


@pytest.mark.parametrize("f32", [False, True], ids=["bf16", "f32"])
@pytest.mark.parametrize("masked", [False, True], ids=["all", "acgt"])
@pytest.mark.parametrize("top_k,top_p,temperature,sigma", SETTINGS)
def test_exact_tokens(top_k, top_p, temperature, sigma, masked, f32):
    n, seed = 4096, 20240 + top_k
    rows = rows_bf16(n, sigma, seed=int(top_k * 7 + sigma))
    mask = acgt_mask() if masked else None
    allow = ops().pack_allow_mask(mask, DEV) if masked else None
    dev_rows = (rows.float() if f32 else rows).to(DEV)
    stream = torch.arange(n, dtype=torch.int64) * 3 + 1
    count = (torch.arange(n, dtype=torch.int64) * 5) % 1000
    full = None
    for S in (4096, 32, 5, 1):
        k, p, t = params(S, top_k, top_p, temperature)
        cnt = count[:S].to(DEV)
        ids, _ = ops().sample_rows(dev_rows[:S], k, p, t, seed, stream=stream[:S].to(DEV), count=cnt, allow=allow)
        torch.cuda.synchronize()
        assert torch.equal(cnt.cpu(), count[:S] + 1)
        ids = ids.cpu()
        assert int(ids.min()) >= 0 and int(ids.max()) < 512
        out, bad = accept(rows[:S], ids, top_k, top_p, temperature, mask, seed, stream[:S].numpy(), count[:S].numpy())
        if S == 4096:
            full = ids
            share = out.float().mean().item()
            print(f"[exact tokens k={top_k} p={top_p} T={temperature} sigma={sigma} mask={masked} f32={f32}] rows left out "
                  f"{100 * share:.2f} %, rejected {int(bad.sum())}")
            assert share <= 0.04, share
        assert int(bad.sum()) == 0, (S, torch.nonzero(bad).flatten()[:8].tolist())
        assert torch.equal(ids, full[:S]), S                          # a row's token does not depend on the rows around it
    # greedy: arg-max of what the mask leaves, lowest id on ties (bf16 rows have ties)
    k, p, t = params(n, 1, top_p, temperature)
    ids, _ = ops().sample_rows(dev_rows, k, p, t, seed, allow=allow)
    ref = rows.float() if mask is None else rows.float().masked_fill(~mask[None, :], float("-inf"))
    want = torch.sort(ref, dim=-1, descending=True, stable=True)[1][:, 0]
    assert torch.equal(ids.cpu(), want)


def test_distribution_of_one_row():
    top_k, top_p, temperature = 50, 0.9, 0.8
    row = rows_bf16(1, 3.0, seed=99)
    assert not bool(undecidable(row, top_k, top_p, temperature, None)[0])
    n = 2 ** 18
    k, p, t = params(n, top_k, top_p, temperature)
    ids, _ = ops().sample_rows(row.to(DEV).expand(n, 512).contiguous(), k, p, t, 1234,
                               stream=torch.arange(n, dtype=torch.int64, device=DEV))
    freq = torch.bincount(ids.cpu(), minlength=512).double() / n
    order, cdf, n_kept = H.seeded_distribution(row, top_k, top_p, temperature)
    prob = torch.zeros(512, dtype=torch.float64)
    prob[order[0]] = torch.diff(cdf[0], prepend=torch.zeros(1, dtype=torch.float64))
    bound = 5 * torch.sqrt(prob * (1 - prob) / n) + 2.0 ** -14
    worst = ((freq - prob).abs() / bound).max().item()
    print(f"[distribution] {int(n_kept[0])} tokens kept, worst |freq - p| / bound = {worst:.3f}")
    assert ((freq - prob).abs() <= bound).all()
    assert freq[order[0, int(n_kept[0]):]].sum().item() == 0.0        # nothing outside the kept set, ever


def test_keying_follows_stream_and_count_not_the_slot():
    S, seed = 4096, 77
    rows = rows_bf16(S, 3.0, seed=5).to(DEV)
    k, p, t = params(S, 50, 0.7, 1.0)
    stream = torch.arange(S, dtype=torch.int64, device=DEV) + 10
    count0 = (torch.arange(S, dtype=torch.int64, device=DEV) * 7) % 50
    active = (torch.arange(S, device=DEV) % 3 != 1)
    cnt = count0.clone()
    a, _ = ops().sample_rows(rows, k, p, t, seed, stream=stream, count=cnt)
    assert torch.equal(cnt, count0 + 1)
    cnt = count0.clone()
    b, _ = ops().sample_rows(rows, k, p, t, seed, stream=stream, count=cnt)
    assert torch.equal(a, b)                                          # same (seed, stream, count): bit for bit
    perm = torch.randperm(S, generator=torch.Generator().manual_seed(1)).to(DEV)
    cnt = count0[perm].clone()
    c, _ = ops().sample_rows(rows[perm].contiguous(), k, p, t, seed, stream=stream[perm].contiguous(), count=cnt)
    assert torch.equal(c, a[perm])                                    # the draw travels with the sample
    cnt = count0.clone()
    d, _ = ops().sample_rows(rows, k, p, t, seed, stream=stream, count=cnt, active=active)
    assert torch.equal(cnt, count0 + active.long())
    assert torch.equal(d[active], a[active])
    e, _ = ops().sample_rows(rows, k, p, t, seed + 1, stream=stream, count=count0.clone())
    assert (e != a).float().mean().item() > 0.2                       # another seed, other draws
    f, _ = ops().sample_rows(rows, k, p, t, seed, stream=stream, count=count0 + 1)
    assert (f != a).float().mean().item() > 0.2                       # the next draw of the same stream


def test_outputs_logprob_history_and_inactive_rows():
    S, L, seed = 257, 6, 3
    rows = rows_bf16(S, 6.0, seed=8)
    for f32 in (False, True):
        dev_rows = (rows.float() if f32 else rows).to(DEV)
        k, p, t = params(S, 4, 0.9, 0.7)
        count0 = (torch.arange(S, dtype=torch.int64) % (L + 2)) - 1                  # -1 and L: outside the history, nothing recorded
        active = (torch.arange(S) % 5 != 2)
        cnt = count0.to(DEV)
        ids = torch.full((S,), -7, dtype=torch.int64, device=DEV)
        lp = torch.full((S,), 123.0, dtype=torch.float32, device=DEV)
        hid = torch.full((S, L), -9, dtype=torch.int64, device=DEV)
        hlg = torch.full((S, L, 512), 777.0, dtype=torch.float32, device=DEV)
        ops().sample_rows(dev_rows, k, p, t, seed, count=cnt, active=active.to(DEV), ids_out=ids, logprob_out=lp, hist_ids=hid,
                          hist_logits=hlg)
        torch.cuda.synchronize()
        ids, lp, hid, hlg, cnt = ids.cpu(), lp.cpu(), hid.cpu(), hlg.cpu(), cnt.cpu()
        assert torch.equal(cnt, count0 + active.long())
        assert (ids[~active] == -7).all() and (lp[~active] == 123.0).all()           # inactive rows: untouched
        want_hid = torch.full((S, L), -9, dtype=torch.int64)
        want_hlg = torch.full((S, L, 512), 777.0)
        rec = active & (count0 >= 0) & (count0 < L)
        r = torch.nonzero(rec).flatten()
        want_hid[r, count0[r]] = ids[r]
        want_hlg[r, count0[r]] = rows.float()[r]
        assert torch.equal(hid, want_hid) and torch.equal(hlg, want_hlg)             # the canaries around them still stand
        # log-probability of the token under the unfiltered row: fp64 yardstick, tolerance 4 x the error of the same formula in fp32 torch
        a = torch.nonzero(active).flatten()
        ref = torch.log_softmax(rows.double(), -1)[a, ids[a]]
        x = dev_rows.float()
        mx = x.max(-1, keepdim=True)[0]
        lsm32 = x - (mx + (x - mx).exp().sum(-1, keepdim=True).log())
        err32 = (lsm32.cpu()[a, ids[a]].double() - ref).abs().max().item()
        err = (lp[a].double() - ref).abs().max().item()
        print(f"[logprob f32={f32}] kernel max |err| {err:.3e}, fp32 torch restatement {err32:.3e}")
        assert err <= 4 * err32, (err, err32)


def test_capture_in_a_graph_equals_eager_launches():
    S, L, seed, n = 32, 9, 11, 8
    rows = rows_bf16(S, 3.0, seed=21).to(DEV)
    k, p, t = params(S, 50, 0.7, 1.0)
    stream = torch.arange(S, dtype=torch.int64, device=DEV)

    def state():
        return (torch.zeros(S, dtype=torch.int64, device=DEV), torch.zeros(S, dtype=torch.int64, device=DEV),
                torch.zeros(S, dtype=torch.float32, device=DEV), torch.full((S, L), -1, dtype=torch.int64, device=DEV),
                torch.zeros(S, L, 512, dtype=torch.float32, device=DEV))
    cnt, ids, lp, hid, hlg = state()
    ops().sample_rows(rows, k, p, t, seed, stream=stream, count=cnt, ids_out=ids, logprob_out=lp, hist_ids=hid, hist_logits=hlg)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ops().sample_rows(rows, k, p, t, seed, stream=stream, count=cnt, ids_out=ids, logprob_out=lp, hist_ids=hid, hist_logits=hlg)
    for _ in range(n - 1):
        g.replay()
    torch.cuda.synchronize()
    cnt2, ids2, lp2, hid2, hlg2 = state()
    for _ in range(n):
        ops().sample_rows(rows, k, p, t, seed, stream=stream, count=cnt2, ids_out=ids2, logprob_out=lp2, hist_ids=hid2, hist_logits=hlg2)
    torch.cuda.synchronize()
    assert (cnt == n).all() and torch.equal(cnt, cnt2)
    assert torch.equal(hid, hid2) and torch.equal(ids, ids2) and torch.equal(lp, lp2) and torch.equal(hlg, hlg2)
    assert (hid[:, :n] >= 0).all() and (hid[:, n:] == -1).all()
    assert len({tuple(col.tolist()) for col in hid[:, :n].T.cpu()}) > 1                # the draws differ from step to step
