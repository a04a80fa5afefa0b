#!/usr/bin/env python
"""Times the paged KV cache against the contiguous cache, legs alternated in one process (not part of bench.py).

    python tools/bench_paged_kv.py [--legs kernel,append,pool,mixed] [--runs 3] [--warmup 1] [--slots 32] [--prompt-len 8192] [--tokens 128]
                                   [--mixed-long 32768] [--mixed-short 1024] [--mixed-tokens 128] [--page-tokens 256] [--small]
                                   [--tree PATH --label NAME --layouts contiguous]

kernel   evo_attn_decode_paged_bf16 beside evo_attn_decode_bf16 at H = 32, the query at the last key, default splits, at 1 x 8,192,
         32 x 8,192 and 1 x 131,072 keys; identity and random page maps, page_tokens 64 and 256; device events, microseconds.
append   the fused rotary + append launch beside its sibling at 8 and 32 rows.
pool     DecodePool, --slots slots, evo-1-8k dimensions, synthetic weights, prompts of --prompt-len nt, one sample each, --tokens tokens:
         the median device time of a captured step, tokens / s over the whole job, stats["kv_bytes"]; contiguous and paged alternated.
mixed    the same with ONE prompt of --mixed-long nt among slots - 1 prompts of --mixed-short nt: what the paged pool is for.
Every figure is the median of --runs timed repetitions after --warmup untimed ones, with (min, max) beside it: the contiguous leg's own
(min, max) in the same call is the yardstick's spread.  One JSON line, with the HBM copy probe of the run.
--tree PATH imports evo_amd from another checkout (with its own build of the library) and --layouts contiguous restricts the pool legs to
the default cache: the parent commit's tree, which has no paged cache, run as a second process of the same call."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def med(v, digits=2):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="kernel,append,pool")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--prompt-len", type=int, default=8192)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--mixed-long", type=int, default=32768)
    ap.add_argument("--mixed-short", type=int, default=1024)
    ap.add_argument("--mixed-tokens", type=int, default=128)
    ap.add_argument("--page-tokens", type=int, default=256)
    ap.add_argument("--tree", default=None, help="import evo_amd from this checkout instead of the one the tool lives in")
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--layouts", default="contiguous,paged")
    ap.add_argument("--small", action="store_true", help="the 4-layer test model instead of the 7B dimensions (a rehearsal, not a measurement)")
    args = ap.parse_args(argv)
    legs = [x for x in args.legs.split(",") if x]
    layouts = [x for x in args.layouts.split(",") if x]
    sys.path.insert(0, os.path.abspath(args.tree) if args.tree else HERE)
    import numpy as np
    import torch
    import evo_amd
    from evo_amd import ops as evo_ops
    from evo_amd.pool import DecodePool
    from evo_amd.tokenizer import CharLevelTokenizer
    if not torch.cuda.is_available():
        raise SystemExit("bench_paged_kv: needs the GPU (no CPU timing path)")
    dev = "cuda:0"
    tok = CharLevelTokenizer(512)
    ops = evo_ops.default_ops()
    out = {"tree": args.label, "evo_amd": os.path.relpath(os.path.dirname(os.path.abspath(evo_amd.__file__))), "runs": args.runs, "warmup": args.warmup}

    def ev_ms(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def alternate(fns, reps):
        """{name: [ms per call]}: the legs alternated, --warmup untimed rounds first."""
        t = {k: [] for k in fns}
        for it in range(args.warmup + args.runs):
            for name, fn in fns.items():
                ms = ev_ms(fn, reps)
                if it >= args.warmup:
                    t[name].append(ms)
        return t

    H = 32
    if "kernel" in legs or "append" in legs:
        from evo_amd.sh.cache import PagedKV

        def paged_copy(kv, pt, kind, seed):
            """kv [B, n, 2, H, 128] (n % pt == 0) as a PagedKV under an identity or a random page map."""
            B, n = kv.shape[:2]
            w = n // pt
            ids = torch.arange(B * w) if kind == "identity" else torch.randperm(B * w, generator=torch.Generator().manual_seed(seed))
            ids = (ids + 1).view(B, w)
            pages = torch.zeros(1 + B * w, pt, 2, H, 128, dtype=kv.dtype, device=dev)
            pages[ids.reshape(-1).to(dev)] = kv.view(B * w, pt, 2, H, 128)
            return PagedKV(pages, ids.to(torch.int32).to(dev))

    if "kernel" in legs:
        out["kernel"] = []
        for B, n in ((1, 8192), (32, 8192), (1, 131072)):
            g = torch.Generator(device=dev).manual_seed(n + B)
            q = torch.randn(B, 1, H, 128, generator=g, device=dev).bfloat16()
            kv = torch.randn(B, n, 2, H, 128, generator=g, device=dev).bfloat16()
            pos = torch.full((B,), n - 1, dtype=torch.int64, device=dev)
            want = ops.attention_decode(q, kv[:, :, 0], kv[:, :, 1], pos=pos)
            row = {"B": B, "keys": n, "H": H, "bytes_read": B * n * 2 * H * 128 * 2}
            for pt in (64, 256):
                recs = {kind: paged_copy(kv, pt, kind, n + pt) for kind in ("identity", "random")}
                fns = {"contiguous": lambda: ops.attention_decode(q, kv[:, :, 0], kv[:, :, 1], pos=pos)}
                for kind, rec in recs.items():
                    fns[kind] = (lambda rec: lambda: ops.attention_decode_paged(q, rec, pos))(rec)
                    assert torch.equal(fns[kind](), want), (B, n, pt, kind)          # the same keys, positions and splits: the same bits
                t = alternate(fns, 20 if B * n <= 65536 else 8)
                c = statistics.median(t["contiguous"])
                row[f"page_tokens_{pt}"] = {**{k + "_us": med([1e3 * x for x in v]) for k, v in t.items()},
                                            **{k + "_over_contiguous": round(statistics.median(t[k]) / c, 3) for k in recs}}
                del recs, fns
                torch.cuda.empty_cache()
            out["kernel"].append(row)
            del q, kv
            torch.cuda.empty_cache()

    if "append" in legs:
        out["append"] = []
        inv = (1.0 / (10000.0 ** (torch.arange(0, 128, 2, dtype=torch.float32, device=dev) / 128))).contiguous()
        for B in (8, 32):
            cap = 8192
            g = torch.Generator(device=dev).manual_seed(B)
            qkv = torch.randn(B, 1, 3, H, 128, generator=g, device=dev).bfloat16()
            kv = torch.zeros(B, cap, 2, H, 128, dtype=torch.bfloat16, device=dev)
            rec = paged_copy(kv, args.page_tokens, "random", B)
            pos = torch.randint(0, cap, (B,), generator=g, device=dev)
            a, b = qkv.clone(), qkv.clone()
            fns = {"contiguous": lambda: ops.rope_append_decode(a, kv, pos, inv, 1.0, q_scale=ops.attn_q_scale(128)),
                   "paged": lambda: ops.rope_append_decode_paged(b, rec, pos, inv, 1.0, q_scale=ops.attn_q_scale(128))}
            t = alternate(fns, 200)
            out["append"].append({"rows": B, "H": H, "page_tokens": args.page_tokens, **{k + "_us": med([1e3 * x for x in v]) for k, v in t.items()}})
            del kv, rec
            torch.cuda.empty_cache()

    def model_of(name):
        if args.small:
            from evo_amd.sh.model import StripedHyena
            from evo_amd.synthetic import synthetic_state_dict
            cfg = dict(vocab_size=512, hidden_size=512, num_layers=4, attn_layer_idxs=[1], num_attention_heads=4)
            m = StripedHyena(cfg)
            m.load_state_dict(synthetic_state_dict(m, seed=0), strict=True)
            m.to_bfloat16_except_poles_residues()
            return m.to(dev).eval()
        return evo_amd.Evo(name, device=dev, weights="synthetic").model.eval()

    def pool_leg(model, n_slots, prompts, n_tokens):
        res = {lay: {"s": [], "step_ms": [], "kv_bytes": None, "stats": None} for lay in layouts}
        for it in range(args.warmup + args.runs):
            for lay in layouts:
                gc.collect()
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                pool = DecodePool(model, tok, n_slots=n_slots, top_k=4, top_p=1.0, temperature=0.7, device=dev, use_graph=True, seed=it,
                                  **({} if lay == "contiguous" else {"kv_paged": True, "kv_page_tokens": args.page_tokens}))
                marks, step = [], pool._step_sampled

                def timed_step():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    step()
                    e1.record()
                    marks.append((e0, e1))
                pool._step_sampled = timed_step
                t0 = time.perf_counter()
                pool.generate(prompts, n_tokens=n_tokens, n_sample_per_prompt=1)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if it >= args.warmup:
                    res[lay]["s"].append(dt)
                    res[lay]["step_ms"].append(statistics.median(a.elapsed_time(b) for a, b in marks[2:]))     # (steps 0, 1: eager, capture)
                    res[lay]["kv_bytes"] = pool.stats["kv_bytes"]
                    res[lay]["stats"] = {k: v for k, v in pool.stats.items() if k.startswith("kv_page")}
                pool._step_sampled = step = None
                del pool, marks
        n_gen = len(prompts) * n_tokens
        return {lay: {"tokens_per_s": round(n_gen / statistics.median(r["s"]), 1), "job_s": med(r["s"], 3), "step_ms": med(r["step_ms"], 4),
                      "kv_bytes": r["kv_bytes"], **(r["stats"] or {})} for lay, r in res.items()}

    rng = np.random.default_rng(0)
    if "pool" in legs or "mixed" in legs:
        model = model_of("evo-1-8k-base")
        if "pool" in legs:
            prompts = ["".join(rng.choice(list("ACGT"), size=args.prompt_len)) for _ in range(args.slots)]
            out["pool"] = {"slots": args.slots, "prompt_len": args.prompt_len, "tokens": args.tokens, "page_tokens": args.page_tokens,
                           **pool_leg(model, args.slots, prompts, args.tokens)}
        if "mixed" in legs:
            lens = [args.mixed_long] + [args.mixed_short] * (args.slots - 1)
            prompts = ["".join(rng.choice(list("ACGT"), size=n)) for n in lens]
            out["mixed"] = {"slots": args.slots, "prompt_lens": f"1 x {args.mixed_long} + {args.slots - 1} x {args.mixed_short}",
                            "tokens": args.mixed_tokens, "page_tokens": args.page_tokens, **pool_leg(model, args.slots, prompts, args.mixed_tokens)}
        del model
    gc.collect()
    torch.cuda.empty_cache()
    # the box's own rate beside the figures (bench.py's `box` block: the HBM copy probe)
    n = 1 << 30
    src = torch.empty(n, dtype=torch.uint8, device=dev).random_(0, 256)
    dst = torch.empty_like(src)
    st = torch.cuda.current_stream().cuda_stream
    ev_ms(lambda: ops.lib.evo_probe_copy_f4(src.data_ptr(), dst.data_ptr(), n, st), 3)
    out["box"] = {"hbm_copy_GBs": round(2.0 * n / (ev_ms(lambda: ops.lib.evo_probe_copy_f4(src.data_ptr(), dst.data_ptr(), n, st), 20) * 1e-3) / 1e9, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
