#!/usr/bin/env python
"""What k-mer repeat control costs, measured in one process with the baseline beside it:

  * the launch alone: `evo_repeat_rows_f32` at S = 8 and S = 32 rows, k = 8 over ACGT (65,536 counts a row), on bf16 logits with a token
    fed and the end rule armed at a fraction no row reaches; device events around every launch, `--launches` launches per repetition.  An
    empty-stream event pair is timed the same way beside it: what an event pair costs with nothing between;
  * the captured step: the pool at `--slots` slots on tools/bench_generate.py's mix of prompts (lengths 0.5x ... 1x `--prompt`) on the
    job-control path (per-prompt limits) without `repeat` against the same call with `RepeatControl(k=8, penalty=0.0)` -- zero levels, so
    both legs draw the same tokens and run the same steps, and the difference is the launch -- alternated, one warm-up each and then
    `--repeats` timed repetitions.  Reported per leg: the captured step alone (device events around every `_step_sampled`, the median over
    a call's replays), and tok/s of the whole call -- which also holds what a fill pays: the prompt's k-mer counts, the copy of M counts
    into the slot and the one-row launch.

Medians over the repetitions, with (min - max) kept; the yardstick of either comparison is the other leg of the same process.

    python tools/bench_repeat.py --out profiles/repeat_ab.txt"""
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
    """Per-repetition values -> median, min, max."""
    return {"per_repeat": [round(float(v), 4) for v in samples], "median": round(float(np.median(samples)), 4),
            "min": round(float(min(samples)), 4), "max": round(float(max(samples)), 4)}


def launch_alone(S, k, launches, repeats, dev):
    """us per launch of the repeat entry on [S, 512] bf16 logits, and of an empty event pair."""
    from evo_amd.ops import default_ops
    o = default_ops()
    g = torch.Generator().manual_seed(S)
    M = 4 ** k
    logits = (torch.randn(S, 512, generator=g) * 3.0).bfloat16().to(dev)
    st = dict(out=torch.zeros(S, 512, dtype=torch.float32, device=dev), active=torch.ones(S, dtype=torch.bool, device=dev),
              counts=torch.randint(0, 3, (S, M), generator=g, dtype=torch.int32).to(dev), ctx=torch.zeros(S, 2, dtype=torch.int32, device=dev),
              stat=torch.zeros(S, 2, dtype=torch.int64, device=dev),
              levels=torch.tensor([[0, 1, 2, 3, 4, 4, 4, 4]] * S, dtype=torch.float32, device=dev))
    end = dict(end_num=torch.full((S,), 1023, dtype=torch.int32, device=dev), end_min_tokens=1 << 40, count=torch.zeros(S, dtype=torch.int64, device=dev),
               length=torch.full((S,), -1, dtype=torch.int64, device=dev), finish=torch.zeros(S, dtype=torch.uint8, device=dev))
    alpha = torch.tensor([A, C, G, T], dtype=torch.int32)
    fed = torch.tensor([A, C, G, T], dtype=torch.int64)[torch.randint(0, 4, (S,), generator=g)].to(dev)
    calls = {"repeat": lambda: o.repeat_rows(logits, st["out"], st["active"], st["counts"], st["ctx"], st["stat"], st["levels"], alpha, k,
                                             fed_ids=fed, **end),
             "empty": lambda: None}
    for _ in range(20):                                               # warm-up
        calls["repeat"]()
    torch.cuda.synchronize()
    per_rep = {name: [] for name in calls}
    for rep in range(repeats + 1):                                    # rep 0 = warm-up of the timing loop itself, not kept
        ev = {name: [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(launches)] for name in calls}
        for i in range(launches):
            for name, f in calls.items():
                ev[name][i][0].record()
                f()
                ev[name][i][1].record()
        torch.cuda.synchronize()
        if rep:
            for name in calls:
                per_rep[name].append(float(np.median([a.elapsed_time(b) for a, b in ev[name]])) * 1e3)
    assert bool(st["active"].all()) and int(st["stat"][0, 0]) == 20 + (repeats + 1) * launches
    return {name: summary(v) for name, v in per_rep.items()}


def step_ab(args, dev):
    """The captured job-control step of one pool shape with and without the repeat launch, alternated."""
    from bench import build_model
    from evo_amd.pool import DecodePool
    from evo_amd.sh.sample import RepeatControl
    from evo_amd.tokenizer import CharLevelTokenizer
    model = build_model(args.model, dev)
    model.decode_graph = True
    tok = CharLevelTokenizer(512)
    rng = np.random.default_rng(7)
    lens = [int(args.prompt * (0.5 + 0.5 * (j % 5) / 4)) for j in range(args.jobs)]
    prompts = ["".join(rng.choice(list("ACGT"), size=n)) for n in lens]
    mk = lambda: DecodePool(model, tok, n_slots=args.slots, top_k=4, top_p=1.0, temperature=0.7, device=dev, use_graph=True, seed=1,
                            allowed_tokens="ACGT")
    runs = {"ctl": (mk(), {}), "ctl_repeat": (mk(), {"repeat": RepeatControl(k=args.k, penalty=0.0)})}
    ms_step, rates, info, marks = {n: [] for n in runs}, {n: [] for n in runs}, {}, {n: [] for n in runs}

    def timed(pool, name):
        step = pool._step_sampled

        def timed_step():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step()
            e1.record()
            marks[name].append((e0, e1))
        return timed_step
    for name, (pool, _) in runs.items():
        pool._step_sampled = timed(pool, name)
    for rep in range(args.repeats + 1):                              # rep 0 = warm-up (allocations, graph capture), not kept
        for name, (pool, kw) in runs.items():
            pool.stats = {k: (0 if isinstance(v, int) and not isinstance(v, bool) else v) for k, v in pool.stats.items()}
            torch.cuda.synchronize()
            marks[name].clear()
            t0 = time.perf_counter()
            pool.generate(prompts, n_tokens=[args.new] * len(prompts), **kw)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            info[name] = {k: pool.stats[k] for k in ("steps", "prefills", "tokens", "polls", "repeat_ends") if k in pool.stats}
            if rep:
                ms_step[name].append(float(np.median([a.elapsed_time(b) for a, b in marks[name]])))      # (replays: rep 0 captured)
                rates[name].append(len(prompts) * args.new / dt)
            print(f"[step slots={args.slots} {name} rep{rep}{' (warm-up)' if not rep else ''}] {dt * 1e3:.0f} ms, "
                  f"{pool.stats['steps']} steps, {len(prompts) * args.new / dt:.0f} tok/s", flush=True)
    a, b = runs["ctl"][0], runs["ctl_repeat"][0]
    assert torch.equal(a.last_ids, b.last_ids) and torch.equal(a.last_logits, b.last_logits)      # zero levels: the same draws, only the cost differs
    assert info["ctl"]["steps"] == info["ctl_repeat"]["steps"]
    out = {n: dict(step_ms=summary(ms_step[n]), tok_per_s=summary(rates[n]), **info[n]) for n in runs}
    out["repeat_minus_ctl_us_per_step"] = round((out["ctl_repeat"]["step_ms"]["median"] - out["ctl"]["step_ms"]["median"]) * 1e3, 2)
    out["repeat_over_ctl_tok_per_s"] = round(out["ctl_repeat"]["tok_per_s"]["median"] / out["ctl"]["tok_per_s"]["median"], 4)
    return dict(model=args.model, slots=args.slots, jobs=len(prompts), prompt_nt=[min(lens), max(lens)], new_tokens=args.new, k=args.k, **out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=200, help="launches per repetition (>= 200)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--rows", default="8,32", help="row counts of the launch alone")
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--model", default="evo-1-8k-base")
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--jobs", type=int, default=64)
    ap.add_argument("--prompt", type=int, default=2048)
    ap.add_argument("--new", type=int, default=128)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--out", default=None, help="append the result line to this file")
    args = ap.parse_args()
    if args.launches < 200 or args.repeats < 2:
        ap.error("--launches >= 200 and --repeats >= 2")
    sys.path.insert(0, ROOT)
    if not torch.cuda.is_available():
        raise SystemExit("bench_repeat.py measures on the GPU; none is visible")
    dev = "cuda:0"
    result = {"launches": args.launches, "repeats": args.repeats, "k": args.k, "launch_us": {}}
    for S in (int(v) for v in args.rows.split(",")):
        result["launch_us"][str(S)] = launch_alone(S, args.k, args.launches, args.repeats, dev)
        print(f"[launch S={S}] {json.dumps(result['launch_us'][str(S)])}", flush=True)
    if not args.skip_step:
        result["step"] = step_ab(args, dev)
    line = json.dumps(result)
    print(line)
    if args.out:
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
