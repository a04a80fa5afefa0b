#!/usr/bin/env python
"""Times the decode pool with ONE stored K/V per prompt (share_prompt_kv) against the replicated pool, in one process (not part of
bench.py), and the grouped decode attention against the shipped entry on a replicated cache.

    python tools/bench_fanout.py [--prompt-lens 1024,8192] [--slots 32] [--samples 8] [--tokens 64] [--runs 5] [--warmup 2]
                                 [--small] [--no-pool] [--no-kernel]

Pool leg: 7B synthetic weights (--small: the 4-layer test model), slots / samples random prompts of each length x --samples samples,
--tokens tokens each, seeded device sampler (the whole step is one captured graph).  share_prompt_kv off and on alternate; the median
of --runs timed runs after --warmup untimed ones: generated tokens / s over the whole job (prefills included), the median device time
of a captured step (events around every replay), and torch.cuda.max_memory_allocated of the leg.
Kernel leg: HipOps.attention_decode_prefix against HipOps.attention_decode on the replicated cache, B = 32, H = 32, a prefix of 8,192
keys and 64 own keys, with the copies of a prompt in adjacent slots and, for comparison, dealt round-robin; achieved bytes / s over the
K/V bytes each form must read.  The rows per workgroup tile are a build constant: an A/B build is another library, picked with
EVO_AMD_LIBNAME and built with EVO_AMD_HIPCC_FLAGS=-DEVO_ATTN_GROUP_ROWS=4.  One JSON line, with the box's own rates beside it."""
import argparse
import json
import os
import re
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--prompt-lens", default="1024,8192")
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-pool", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    args = ap.parse_args(argv)
    import gc
    import numpy as np
    import torch
    import evo_amd
    from evo_amd import ops as evo_ops
    from evo_amd.pool import DecodePool
    from evo_amd.tokenizer import CharLevelTokenizer
    dev = "cuda:0"
    tok = CharLevelTokenizer(512)
    flag = re.search(r"-DEVO_ATTN_GROUP_ROWS=(\d+)", os.environ.get("EVO_AMD_HIPCC_FLAGS", ""))
    group_rows = int(flag.group(1)) if flag else evo_ops.ATTN_GROUP_ROWS
    out = {"group_rows": group_rows, "library": os.environ.get("EVO_AMD_LIBNAME", "libevo_mi355x.so"), "runs": args.runs}
    ops = evo_ops.default_ops()
    ops.attn_group_rows = group_rows

    def ev_ms(fn, reps):
        for _ in range(2):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    # ------------------------------------------------------------------ kernel leg
    if not args.no_kernel:
        B, H, P, own = 32, 32, 8192, 64
        n_prompts = B // args.samples if B % args.samples == 0 else 4
        g = torch.Generator(device=dev).manual_seed(1)
        store = torch.randn(n_prompts, P, 2, H, 128, generator=g, device=dev).bfloat16()
        kv_own = torch.randn(B, own, 2, H, 128, generator=g, device=dev).bfloat16()
        q = torch.randn(B, 1, H, 128, generator=g, device=dev).bfloat16()
        i64 = lambda x: torch.tensor(x, dtype=torch.int64, device=dev)                        # noqa: E731
        adjacent = i64([b // (B // n_prompts) for b in range(B)])
        dealt = i64([b % n_prompts for b in range(B)])
        own_pos, pre_len = i64([own - 1] * B), i64([P] * n_prompts)
        kv_rep = torch.empty(B, P + own, 2, H, 128, dtype=torch.bfloat16, device=dev)

        def fill(rows):
            kv_rep[:, :P] = store[rows]
            kv_rep[:, P:] = kv_own
        pos = i64([P + own - 1] * B)
        legs = {"replicated": lambda: ops.attention_decode(q, kv_rep[:, :, 0], kv_rep[:, :, 1], pos=pos),
                "shared_adjacent": lambda: ops.attention_decode_prefix(q, kv_own[:, :, 0], kv_own[:, :, 1], own_pos, store[:, :, 0], store[:, :, 1],
                                                                       adjacent, pre_len),
                "shared_dealt": lambda: ops.attention_decode_prefix(q, kv_own[:, :, 0], kv_own[:, :, 1], own_pos, store[:, :, 0], store[:, :, 1],
                                                                    dealt, pre_len)}
        fill(adjacent)
        want = legs["replicated"]().float()
        got = legs["shared_adjacent"]().float()
        fill(dealt)
        want_d, got_d = legs["replicated"]().float(), legs["shared_dealt"]().float()
        tk = {k: [] for k in legs}
        for it in range(args.warmup + args.runs):
            for name, fn in legs.items():
                ms = ev_ms(fn, 20)
                if it >= args.warmup:
                    tk[name].append(ms)
        key_bytes = 2 * H * 128 * 2                                                           # K and V of one key, all heads
        need = {"replicated": B * (P + own) * key_bytes, "shared_adjacent": (n_prompts * P + B * own) * key_bytes}
        need["shared_dealt"] = need["shared_adjacent"]
        tiles = (B + group_rows - 1) // group_rows
        streams = {"shared_adjacent": sum(len(set(adjacent[t * group_rows:(t + 1) * group_rows].tolist())) for t in range(tiles)),
                   "shared_dealt": sum(len(set(dealt[t * group_rows:(t + 1) * group_rows].tolist())) for t in range(tiles))}
        out["kernel"] = {"B": B, "H": H, "prefix": P, "own": own, "prompts": n_prompts,
                         "max_abs_diff_vs_replicated": max((got - want).abs().max().item(), (got_d - want_d).abs().max().item()),
                         "prefix_streams": streams,
                         **{name + "_us": round(1e3 * statistics.median(v), 2) for name, v in tk.items()},
                         **{name + "_needed_GBs": round(need[name] / (statistics.median(v) * 1e-3) / 1e9, 1) for name, v in tk.items()},
                         "needed_bytes": need}
        del store, kv_own, kv_rep

    # ------------------------------------------------------------------ pool leg
    if not args.no_pool:
        if args.small:
            from evo_amd.sh.model import StripedHyena
            from evo_amd.synthetic import synthetic_state_dict
            cfg = dict(vocab_size=512, hidden_size=256, num_layers=4, attn_layer_idxs=[2], num_attention_heads=2)
            model = StripedHyena(cfg)
            model.load_state_dict(synthetic_state_dict(model, seed=0), strict=True)
            model.to_bfloat16_except_poles_residues()
            model = model.to(dev)
        else:
            model = evo_amd.Evo("evo-1-8k-base", device=dev, weights="synthetic").model
        model.eval()
        model.ops.attn_group_rows = group_rows
        rng = np.random.default_rng(0)
        n_prompts = max(1, args.slots // args.samples)
        out["pool"] = {"slots": args.slots, "prompts": n_prompts, "samples": args.samples, "tokens": args.tokens, "legs": []}
        for plen in [int(x) for x in args.prompt_lens.split(",") if x]:
            prompts = ["".join(rng.choice(list("ACGT"), size=plen)) for _ in range(n_prompts)]
            res = {False: {"s": [], "step_ms": [], "mem": 0}, True: {"s": [], "step_ms": [], "mem": 0}}
            stats = None
            for it in range(args.warmup + args.runs):
                for share in (False, True):
                    gc.collect()                                     # (the previous leg's pool: its caches must not count here)
                    torch.cuda.synchronize()
                    torch.cuda.empty_cache()
                    torch.cuda.reset_peak_memory_stats()
                    base = torch.cuda.memory_allocated()
                    pool = DecodePool(model, tok, n_slots=args.slots, top_k=4, top_p=1.0, temperature=0.7, device=dev, use_graph=True, seed=it,
                                      share_prompt_kv=share)
                    marks, step = [], pool._step_sampled

                    def timed_step():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        step()
                        e1.record()
                        marks.append((e0, e1))
                    pool._step_sampled = timed_step
                    t0 = time.perf_counter()
                    seqs, _, _ = pool.generate(prompts, n_tokens=args.tokens, n_sample_per_prompt=args.samples)
                    torch.cuda.synchronize()
                    dt = time.perf_counter() - t0
                    if it >= args.warmup:
                        r = res[share]
                        r["s"].append(dt)
                        r["step_ms"].append(statistics.median(a.elapsed_time(b) for a, b in marks[2:]))    # (steps 0, 1: eager, capture)
                        r["mem"] = max(r["mem"], torch.cuda.max_memory_allocated())
                        r["kv"] = sum(t.numel() * t.element_size() for t in pool.ipd["mha"].key_value_memory_dict.values()) \
                            + (sum(t.numel() * t.element_size() for t in pool.store.kv.values()) if share else 0)
                        r["base"] = base
                    if share:
                        stats = dict(pool.stats)
                    pool._step_sampled = step = None                 # (break the cycle pool -> wrapper -> bound method -> pool)
                    del pool, marks
            n_gen = len(prompts) * args.samples * args.tokens
            leg = {"prompt_len": plen, "stats_shared": stats}
            for share, name in ((False, "replicated"), (True, "shared")):
                r = res[share]
                leg[name] = {"tokens_per_s": round(n_gen / statistics.median(r["s"]), 1), "job_s": round(statistics.median(r["s"]), 4),
                             "step_ms": round(statistics.median(r["step_ms"]), 4), "max_memory_allocated": r["mem"], "allocated_before_the_leg": r["base"], "kv_cache_bytes": r["kv"]}
            out["pool"]["legs"].append(leg)

    # the box's own rates beside the figures (bench.py's `box` block: the HBM copy probe and the library GEMM)
    n = 1 << 30
    src = torch.empty(n, dtype=torch.uint8, device=dev).random_(0, 256)
    dst = torch.empty_like(src)
    st = torch.cuda.current_stream().cuda_stream
    copy_gbs = 2.0 * n / (ev_ms(lambda: ops.lib.evo_probe_copy_f4(src.data_ptr(), dst.data_ptr(), n, st), 20) * 1e-3) / 1e9
    del src, dst
    g = torch.Generator(device=dev).manual_seed(2)
    a_ = torch.randn(8192, 8192, generator=g, device=dev).bfloat16()
    b_ = torch.randn(8192, 8192, generator=g, device=dev).bfloat16()
    gemm_tflops = 2.0 * 8192 ** 3 / (ev_ms(lambda: torch.mm(a_, b_), 10) * 1e-3) / 1e12
    out["box"] = {"hbm_copy_GBs": round(copy_gbs, 1), "library_gemm_tflops": round(gemm_tflops, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
