#!/usr/bin/env python
"""BASELINE configs[4]: evo-1-131k-base generation, 8,192-nt prompt -> N new tokens (greedy), recurrent Hyena
state + KV cache, 1 x MI355X.  Reports prefill time and decode ms/token (total minus a prefill-only run).
    python tools/bench_generate.py [--new 256] [--batch 1] [--no-graph]
Pool mode with --seed: the same job with the host sampler (the default path) and with the device sampler (csrc/sample.hip), alternated
in one process -- tok/s, ms/step and the repeat-to-repeat spread of both, optionally as one JSON line (--json).
    python tools/bench_generate.py --pool 8,32 --jobs 64 --seed 1 --repeats 3 --json profiles/sample_bench_line.json"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def sampler_ab(args, model, tok, prompts, slot_counts, dev):
    """Host sampler against device sampler on the same job, alternated: host, device, host, device, ..."""
    from evo_amd.pool import DecodePool
    result = {"model": args.model, "jobs": len(prompts), "prompt_nt": [min(map(len, prompts)), max(map(len, prompts))],
              "new_tokens": args.new, "graph": not args.no_graph, "repeats": args.repeats, "slots": {}}
    for n_slots in slot_counts:
        pools = {"host": DecodePool(model, tok, n_slots=n_slots, top_k=4, top_p=1.0, temperature=0.7, device=dev,
                                    use_graph=not args.no_graph),
                 "device": DecodePool(model, tok, n_slots=n_slots, top_k=4, top_p=1.0, temperature=0.7, device=dev,
                                      use_graph=not args.no_graph, seed=args.seed)}
        times = {k: [] for k in pools}
        steps = {}
        for rep in range(args.repeats + 1):                          # rep 0 = warm-up (allocations, graph capture), not kept
            for name, pool in pools.items():
                pool.stats = {"steps": 0, "prefills": 0, "tokens": 0}
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pool.generate(prompts, n_tokens=args.new)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                steps[name] = pool.stats["steps"]
                if rep:
                    times[name].append(dt)
                print(f"[sampler A/B slots={n_slots} {name} rep{rep}{' (warm-up)' if not rep else ''}] {dt * 1e3:.0f} ms, "
                      f"{len(prompts) * args.new / dt:.0f} tok/s, {dt / steps[name] * 1e3:.3f} ms/step incl. prefills", flush=True)
        row = {}
        for name, ts in times.items():
            med = float(np.median(ts))
            row[name] = {"seconds": [round(t, 4) for t in ts], "median_s": round(med, 4), "tok_per_s": round(len(prompts) * args.new / med, 1),
                         "ms_per_step": round(med / steps[name] * 1e3, 4), "steps": steps[name],
                         "spread": round((max(ts) - min(ts)) / med, 4)}
        row["device_over_host_time"] = round(row["device"]["median_s"] / row["host"]["median_s"], 4)
        row["not_slower_within_host_spread"] = bool(row["device"]["median_s"] <= row["host"]["median_s"] * (1 + row["host"]["spread"]))
        result["slots"][str(n_slots)] = row
        del pools
        torch.cuda.empty_cache()
    line = json.dumps(result)
    print(line)
    if args.json:
        with open(args.json, "w") as f:
            f.write(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompt", type=int, default=8192)
    ap.add_argument("--new", type=int, default=256)
    ap.add_argument("--batch", type=int, default=1)
    ap.add_argument("--model", default="evo-1-131k-base")
    ap.add_argument("--no-graph", action="store_true")
    ap.add_argument("--pool", default="0", help="continuous batching: number of decode slots (0 = off; with --seed a list: 8,32)")
    ap.add_argument("--jobs", type=int, default=16, help="pool mode: number of prompts (lengths vary 0.5x..1x --prompt)")
    ap.add_argument("--seed", type=int, default=None, help="pool mode: A/B of the host sampler against the seeded device sampler")
    ap.add_argument("--repeats", type=int, default=3, help="timed repeats per sampler in the A/B (after one warm-up each)")
    ap.add_argument("--json", default=None, help="A/B: write the result line to this file")
    args = ap.parse_args()
    slot_counts = [int(v) for v in str(args.pool).split(",") if int(v) > 0]
    args.pool = slot_counts[0] if slot_counts else 0
    from bench import build_model
    from evo_amd.generation import Generator
    from evo_amd.tokenizer import CharLevelTokenizer
    dev = "cuda:0"
    model = build_model(args.model, dev)
    model.decode_graph = not args.no_graph
    tok = CharLevelTokenizer(512)
    rng = np.random.default_rng(7)
    ids = torch.from_numpy(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=(args.batch, args.prompt)).astype(np.int64)).to(dev)
    if args.pool:
        from evo_amd.pool import DecodePool
        lens = [int(args.prompt * (0.5 + 0.5 * (j % 5) / 4)) for j in range(args.jobs)]
        prompts = ["".join(rng.choice(list("ACGT"), size=n)) for n in lens]
        if args.seed is not None:
            return sampler_ab(args, model, tok, prompts, slot_counts, dev)
        pool = DecodePool(model, tok, n_slots=args.pool, top_k=4, top_p=1.0, temperature=0.7, device=dev,
                          use_graph=not args.no_graph)
        pool.generate(prompts[:2], n_tokens=4)                 # warm-up (allocations, graph capture)
        for rep in range(2):
            pool.stats = {"steps": 0, "prefills": 0, "tokens": 0}
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            seqs, scores, _ = pool.generate(prompts, n_tokens=args.new)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(f"[pool slots={args.pool} graph={not args.no_graph} rep{rep}] {args.jobs} prompts of {min(lens)}..{max(lens)} nt, "
                  f"{args.new} new tokens each: {dt * 1e3:.0f} ms total, {args.jobs * args.new / dt:.0f} tok/s aggregate "
                  f"({pool.stats['steps']} steps, {dt / max(1, pool.stats['steps']) * 1e3:.2f} ms/step incl. prefills)")
        return
    g = Generator(model, tok, top_k=1, top_p=1.0, temperature=1.0)

    def run(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, scores, cache = g.generate(device=dev, input_ids=ids, num_tokens=n, cached_generation=True,
                                        print_generation=False, stop_at_eos=False)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out, cache

    run(2)                                                     # warm-up
    for rep in range(2):
        t_pre, _, _ = run(1)
        t_all, out, cache = run(1 + args.new)
        t_dec = t_all - t_pre
        print(f"[gen graph={not args.no_graph} rep{rep}] B={args.batch} prompt={args.prompt}: prefill {t_pre * 1e3:.1f} ms "
              f"({args.batch * args.prompt / t_pre:.0f} nt/s); decode {args.new} tok in {t_dec * 1e3:.1f} ms = "
              f"{t_dec / args.new * 1e3:.2f} ms/tok, {args.batch * args.new / t_dec:.1f} tok/s; "
              f"offset={cache['mha'].seqlen_offset} graph_engaged={getattr(model, 'decode_graph_replays', 0) > 0}")


if __name__ == "__main__":
    main()
