#!/usr/bin/env python
"""What constrained generation costs, measured in one process with the baselines beside it:

  * the sampler launch: `evo_sample_rows_ctl_f32` against `evo_sample_rows_dfa_f32` at S = 8 and S = 32 rows, interleaved launch by
    launch, device events around every launch, `--launches` (>= 200) launches of each per repetition, `--repeats` repetitions.  Both draw
    from ACGT on the same logits; the automaton is one state that loops on every letter, so no row ever ends;
  * the pool at 32 slots on tools/bench_generate.py's mix of prompts (lengths 0.5x ... 1x `--prompt`): the unconstrained seeded run against
    the same run under `iupac_template("N" * n)` -- the same draws, plus the table read, the state update and the host's polls --
    alternated, one warm-up each and then `--repeats` timed repetitions.

`--tree PATH` imports `evo_amd` and `bench` from another checkout (built there): the baseline of an A/B against an earlier commit, run as
a process of its own on the same box.  A tree without `sample_rows_dfa` runs the unconstrained halves only.

The margin of every comparison is the run-to-run spread of the baseline, (max - min) / median over its repetitions.

    python tools/bench_constraints.py --out profiles/constraints_ab.txt
    python tools/bench_constraints.py --tree ../parent --label parent --out profiles/constraints_ab.txt"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
A, C, G, T = (ord(c) for c in "ACGT")


def summary(samples):
    """Per-repetition values -> median, min, max and spread = (max - min) / median."""
    med = float(np.median(samples))
    return {"per_repeat": [round(float(v), 4) for v in samples], "median": round(med, 4), "min": round(float(min(samples)), 4),
            "max": round(float(max(samples)), 4), "spread": round(float((max(samples) - min(samples)) / med), 4)}


def launch_ab(S, launches, repeats, dev):
    """us per launch of the control entry and of the automaton entry on the same [S, 512] bf16 logits, launch by launch in turn."""
    from evo_amd.ops import default_ops
    from evo_amd.sh.sample import allowed_mask
    o = default_ops()
    g = torch.Generator().manual_seed(S)
    logits = (torch.randn(S, 512, generator=g) * 3.0).bfloat16().to(dev)
    allow = o.pack_allow_mask(allowed_mask(None, [A, C, G, T]), dev)
    prm = (torch.full((S,), 4, dtype=torch.int32, device=dev), torch.full((S,), 1.0, dtype=torch.float32, device=dev),
           torch.full((S,), 0.7, dtype=torch.float32, device=dev))

    def state():
        return dict(count=torch.zeros(S, dtype=torch.int64, device=dev), active=torch.ones(S, dtype=torch.bool, device=dev),
                    limit=torch.full((S,), 1 << 40, dtype=torch.int64, device=dev), length=torch.full((S,), -1, dtype=torch.int64, device=dev),
                    finish=torch.zeros(S, dtype=torch.uint8, device=dev), stream=torch.arange(S, dtype=torch.int64, device=dev),
                    ids_out=torch.zeros(S, dtype=torch.int64, device=dev), logprob_out=torch.zeros(S, dtype=torch.float32, device=dev))
    st = {"ctl": state()}
    calls = {"ctl": lambda: o.sample_rows_ctl(logits, *prm, 1, allow=allow, **st["ctl"])}
    if hasattr(o, "sample_rows_dfa"):
        st["dfa"] = state()
        dfa = dict(dfa_alphabet=torch.tensor([A, C, G, T], dtype=torch.int32),
                   dfa_next=torch.tensor([[0, 0, 0, 0, -1, -1, -1, -1]], dtype=torch.int32, device=dev),
                   dfa_base=torch.zeros(S, dtype=torch.int64, device=dev), dfa_state=torch.zeros(S, dtype=torch.int32, device=dev))
        calls["dfa"] = lambda: o.sample_rows_dfa(logits, *prm, 1, allow=allow, **st["dfa"], **dfa)
    for _ in range(20):                                               # warm-up
        for f in calls.values():
            f()
    torch.cuda.synchronize()
    per_rep = {k: [] for k in calls}
    for _ in range(repeats):
        ev = {k: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)] for k in calls}
        for i in range(launches):
            for k, f in calls.items():
                ev[k][i][0].record()
                f()
                ev[k][i][1].record()
        torch.cuda.synchronize()
        for k in calls:
            per_rep[k].append(float(np.median([a.elapsed_time(b) for a, b in ev[k]])) * 1e3)
    if "dfa" in st:
        assert torch.equal(st["ctl"]["ids_out"], st["dfa"]["ids_out"]) and torch.equal(st["ctl"]["count"], st["dfa"]["count"])
        assert bool(st["dfa"]["active"].all())
    out = {k: summary(v) for k, v in per_rep.items()}
    if "dfa" in out:
        out["dfa_over_ctl"] = round(out["dfa"]["median"] / out["ctl"]["median"], 4)
        out["within_ctl_spread"] = bool(out["dfa"]["median"] <= out["ctl"]["median"] * (1 + out["ctl"]["spread"]))
    return out


def pool_ab(args, dev):
    """tok/s of the pool at `--slots` slots: unconstrained against iupac_template("N" * n), alternated."""
    from bench import build_model
    from evo_amd.pool import DecodePool
    from evo_amd.tokenizer import CharLevelTokenizer
    model = build_model(args.model, dev)
    model.decode_graph = True
    tok = CharLevelTokenizer(512)
    rng = np.random.default_rng(7)
    lens = [int(args.prompt * (0.5 + 0.5 * (j % 5) / 4)) for j in range(args.jobs)]
    prompts = ["".join(rng.choice(list("ACGT"), size=n)) for n in lens]
    mk = lambda: DecodePool(model, tok, n_slots=args.slots, top_k=4, top_p=1.0, temperature=0.7, device=dev, use_graph=True, seed=1,
                            allowed_tokens="ACGT")
    runs = {"free": (mk(), {})}
    try:
        from evo_amd.constraints import iupac_template
        runs["template_N"] = (mk(), {"constraints": iupac_template("N" * args.new)})
    except ImportError:
        pass
    rates, info = {k: [] for k in runs}, {}
    for rep in range(args.repeats + 1):                              # rep 0 = warm-up (allocations, graph capture), not kept
        for name, (pool, kw) in runs.items():
            pool.stats = {k: 0 for k in pool.stats}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pool.generate(prompts, n_tokens=args.new, **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            info[name] = {k: pool.stats[k] for k in ("steps", "prefills", "tokens", "polls", "constraint_ends") if k in pool.stats}
            if rep:
                rates[name].append(len(prompts) * args.new / dt)
            print(f"[pool slots={args.slots} {name} rep{rep}{' (warm-up)' if not rep else ''}] {dt * 1e3:.0f} ms, "
                  f"{len(prompts) * args.new / dt:.0f} tok/s, {pool.stats['steps']} steps", flush=True)
    if len(runs) == 2:
        assert torch.equal(runs["free"][0].last_ids, runs["template_N"][0].last_ids)      # the same draws: only the cost differs
    out = {k: dict(tok_per_s=summary(v), **info[k]) for k, v in rates.items()}
    if len(runs) == 2:
        free, con = out["free"]["tok_per_s"], out["template_N"]["tok_per_s"]
        out["template_over_free"] = round(con["median"] / free["median"], 4)
        out["within_free_spread"] = bool(con["median"] >= free["median"] * (1 - free["spread"]))
    return dict(model=args.model, slots=args.slots, jobs=len(prompts), prompt_nt=[min(lens), max(lens)], new_tokens=args.new, **out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--tree", default=ROOT, help="the checkout to import evo_amd and bench from (default: this one)")
    ap.add_argument("--label", default="this tree", help="what the result line calls the tree")
    ap.add_argument("--launches", type=int, default=200, help="launches of each entry per repetition (>= 200)")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--rows", default="8,32", help="row counts of the launch A/B")
    ap.add_argument("--model", default="evo-1-8k-base")
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--jobs", type=int, default=64)
    ap.add_argument("--prompt", type=int, default=2048)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--skip-pool", action="store_true")
    ap.add_argument("--out", default=None, help="append the result line to this file")
    args = ap.parse_args()
    if args.launches < 200 or args.repeats < 2:
        ap.error("--launches >= 200 and --repeats >= 2")
    sys.path.insert(0, os.path.abspath(args.tree))
    dev = "cuda:0"
    result = {"tree": args.label, "launches": args.launches, "repeats": args.repeats, "launch_us": {}}
    for S in (int(v) for v in args.rows.split(",")):
        result["launch_us"][str(S)] = launch_ab(S, args.launches, args.repeats, dev)
        print(f"[launch S={S}] {json.dumps(result['launch_us'][str(S)])}", flush=True)
    if not args.skip_pool:
        result["pool"] = pool_ab(args, dev)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
