#!/usr/bin/env python
"""BASELINE configs[4]: evo-1-131k-base generation, 8,192-nt prompt -> N new tokens (greedy), recurrent Hyena
state + KV cache, 1 x MI355X.  Reports prefill time and decode ms/token (total minus a prefill-only run).
    python tools/bench_generate.py [--new 256] [--batch 1] [--no-graph]
Pool mode with --seed: the same job with the host sampler (the default path) and with the device sampler (csrc/sample.hip), alternated
in one process -- tok/s, ms/step and the repeat-to-repeat spread of both, optionally as one JSON line (--json).
    python tools/bench_generate.py --pool 8,32 --jobs 64 --seed 1 --repeats 3 --json profiles/sample_bench_line.json
Pool mode with a stop rule (--stop-tokens / --stop-sequences): the same job at fixed length (today's path) and with jobs
that end on their own, alternated in one process, for every --poll-every value -- pooled steps, seconds, jobs/s, device and host bytes.
    python tools/bench_generate.py --model evo-1-8k-base --pool 32 --jobs 64 --prompt 2048 --new 1024 --seed 1 --allowed-tokens ACGT \
        --stop-sequences TAA,TAG,TGA --stop-frame 3 --poll-every 1,4,8,16 --temperature 8 --json profiles/stop_bench_line.json"""
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


def stop_ab(args, model, tok, prompts, n_slots, dev):
    """Fixed length (evo_sample_rows_f32) against jobs that end on their own (evo_sample_rows_ctl_f32), alternated: fixed, stop, fixed, ..."""
    from evo_amd.pool import DecodePool
    rule = dict(stop_frame=args.stop_frame, return_logits=not args.scores_only)
    if args.stop_tokens:
        rule["stop_tokens"] = args.stop_tokens
    if args.stop_sequences:
        rule["stop_sequences"] = [p for p in args.stop_sequences.split(",") if p]
    polls = [int(v) for v in str(args.poll_every).split(",")]
    mk = lambda **kw: DecodePool(model, tok, n_slots=n_slots, top_k=4, top_p=1.0, temperature=args.temperature, device=dev,
                                 use_graph=not args.no_graph, seed=args.seed or 0, allowed_tokens=args.allowed_tokens, **kw)
    pools = {"fixed": mk()}
    pools.update({f"stop_poll{p}": mk(poll_every=p) for p in polls})
    result = {"model": args.model, "jobs": len(prompts), "prompt_nt": [min(map(len, prompts)), max(map(len, prompts))], "limit": args.new,
              "slots": n_slots, "temperature": args.temperature, "allowed_tokens": args.allowed_tokens, "rule": {k: v for k, v in rule.items()},
              "graph": not args.no_graph, "repeats": args.repeats, "runs": {}}
    times, info = {k: [] for k in pools}, {}
    for rep in range(args.repeats + 1):                              # rep 0 = warm-up (allocations, graph capture), not kept
        for name, pool in pools.items():
            pool.stats = {k: 0 for k in pool.stats}
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            t0 = time.perf_counter()
            pool.generate(prompts, n_tokens=args.new, **({} if name == "fixed" else rule))
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            hist = sum(t.numel() * t.element_size() for t in (pool.hist_ids, pool.hist_logits, getattr(pool, "hist_logprob", None)) if t is not None)
            host = sum(t.numel() * t.element_size() for t in (pool.last_ids, pool.last_logits, getattr(pool, "last_logprobs", None)) if t is not None)
            info[name] = dict(pool.stats, device_history_bytes=hist, host_result_bytes=host, device_peak_bytes=torch.cuda.max_memory_allocated())
            if name != "fixed":
                info[name]["mean_length"] = round(float(np.mean(pool.last_lengths)), 1)
            if rep:
                times[name].append(dt)
            print(f"[stop A/B slots={n_slots} {name} rep{rep}{' (warm-up)' if not rep else ''}] {dt * 1e3:.0f} ms, {pool.stats['steps']} steps, "
                  f"{len(prompts) / dt:.2f} jobs/s", flush=True)
    for name, ts in times.items():
        med = float(np.median(ts))
        result["runs"][name] = dict(info[name], seconds=[round(t, 4) for t in ts], median_s=round(med, 4), jobs_per_s=round(len(prompts) / med, 3),
                                    spread=round((max(ts) - min(ts)) / med, 4))
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
    ap.add_argument("--allowed-tokens", default=None, help="pool mode with a stop rule: characters that may be drawn")
    ap.add_argument("--stop-tokens", default=None, help="pool mode: characters that end a job (A/B against the fixed-length job)")
    ap.add_argument("--stop-sequences", default=None, help="pool mode: comma-separated stop patterns, e.g. TAA,TAG,TGA")
    ap.add_argument("--stop-frame", type=int, default=1)
    ap.add_argument("--scores-only", action="store_true", help="stop A/B: the job-control runs keep no logits")
    ap.add_argument("--poll-every", default="8", help="stop A/B: the poll intervals to compare, e.g. 1,4,8,16")
    ap.add_argument("--temperature", type=float, default=0.7, help="stop A/B: sampling temperature (synthetic weights repeat their last "
                                                                   "token at 0.7; a high value spreads the draws)")
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
        if args.stop_tokens or args.stop_sequences:
            return stop_ab(args, model, tok, prompts, args.pool, dev)
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
