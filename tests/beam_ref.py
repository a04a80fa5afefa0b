"""Helpers of the beam-search tests (no tests here): the CPU oracle backend with the optional group "beam", and a naive beam search
that shares nothing with the pool.

`BeamOracleOps`: the fp64 oracle ops of the ragged / constraint host tests plus `beam_select` -- the written specification
(evo_amd/sh/sample.py) applied in place, history and step counters as the C entry documents them -- and `gather_rows`, an `index_select`
per registered tensor (of a per-token tensor only the first own_pos[parent] + 1 tokens, as the kernel)."""
import torch

from evo_amd.sh import sample as H
from test_constraints_host import DfaOracleOps
from test_ragged_prefill_host import RaggedOracleOps
from test_stop_host import _bits


class BeamOracleOps(DfaOracleOps, RaggedOracleOps):
    beam_cum_dtype = torch.float64                                    # the pool keeps cum (and the prefill's last logits) in the oracle's precision

    def __init__(self, act=torch.float64):
        super().__init__(act)
        self.beam_calls = {"select": 0, "gather": 0, "moved": 0}
        self.select_log = None                                        # a list: every call's (logits, state before) is appended

    def beam_select(self, logits, cum, ended, length, ids, parent, beam_width, group_active=None, allow=None, stop_mask=None,
                    hist_parent=None, hist_ids=None, hist_cum=None, step=None, t=-1):
        self.beam_calls["select"] += 1
        W, S = int(beam_width), logits.shape[0]
        flat = ids.view(-1)
        if self.select_log is not None:
            self.select_log.append((logits.clone(), cum.clone(), ended.clone(), length.clone(), flat.clone(),
                                    None if group_active is None else group_active.clone()))
        p, i, c, e, n = H.beam_select(logits, cum, ended, length, flat, W, group_active, _bits(allow), _bits(stop_mask), dtype=torch.float64)
        parent.copy_(p)
        flat.copy_(i)
        cum.copy_(c.to(cum.dtype))
        ended.copy_(e.to(ended.dtype))
        length.copy_(n)
        for g in range(S // W):
            if group_active is not None and not bool(group_active[g]):
                continue
            col = int(step[g]) if step is not None else int(t)
            if hist_parent is not None and 0 <= col < hist_parent.shape[1]:
                rows = slice(g * W, g * W + W)
                hist_parent[rows, col] = p[rows].to(hist_parent.dtype)
                hist_ids[rows, col] = i[rows]
                if hist_cum is not None:
                    hist_cum[rows, col] = c[rows].to(hist_cum.dtype)
            if step is not None:
                step[g] = col + 1

    def gather_table(self, fixed, per_token=()):
        return {"fixed": list(fixed), "per_token": list(per_token)}

    def gather_rows(self, tab, parent, own_pos):
        self.beam_calls["gather"] += 1
        S = parent.shape[0]
        p = parent.clamp(0, S - 1)
        self.beam_calls["moved"] += int((p != torch.arange(S)).sum())
        for x in tab["fixed"]:
            x.copy_(x.index_select(0, p))
        for x in tab["per_token"]:
            old = x.clone()
            for s in range(S):
                if int(p[s]) != s:
                    n = min(max(int(own_pos[p[s]]) + 1, 0), x.shape[1])
                    x[s, :n] = old[p[s], :n]


def toy_model(ops):
    from oracle.stripedhyena_ref import RefConfig, make_synthetic_state_dict
    from evo_amd.sh.model import StripedHyena
    from test_ragged_prefill_host import SMALL
    sd = make_synthetic_state_dict(RefConfig.from_dict(SMALL), seed=3)
    m = StripedHyena(dict(SMALL), ops=ops)
    m.load_state_dict({k: (v.double() if v.dtype == torch.bfloat16 else v) for k, v in sd.items()})
    return m


def naive_beam_search(m, prompt: str, n_tokens: int, W: int, allowed: str, stop: str = ""):
    """Beam search that re-forwards every hypothesis from scratch each step (no caches, no reparenting): -> [(tokens, score, ended)] in
    rank order.  Ranking: score descending, then the parent's rank ascending, then token ascending."""
    allow = sorted(ord(ch) for ch in allowed)
    stops = {ord(ch) for ch in stop}
    hyps = [([], 0.0, False)]
    with torch.inference_mode():
        for _ in range(n_tokens):
            if all(e for _, _, e in hyps):
                break
            cands = []
            for b, (toks, cum, e) in enumerate(hyps):
                if e:
                    cands.append((-cum, b, -1, toks, cum, True))
                    continue
                row = m(torch.tensor([list(prompt.encode()) + toks]))[0][0, -1].double()
                lse = torch.logsumexp(row, -1)
                for v in allow:
                    sc = float(torch.tensor(cum, dtype=torch.float64) + (row[v] - lse))
                    cands.append((-sc, b, v, toks + [v], sc, v in stops))
            cands.sort(key=lambda c: c[:3])
            hyps = [(c[3], c[4], c[5]) for c in cands[:W]]
    return hyps
