#!/usr/bin/env python
"""Times the FP8 (e4m3fn) KV cache against the bf16 cache, legs alternated in one process (not part of bench.py).

    python tools/bench_kv_fp8.py [--legs kernel,append,pool,long,quality] [--runs 5] [--warmup 2] [--slots 32] [--prompt-len 8192]
                                 [--tokens 128] [--long-len 131072] [--long-tokens 32] [--small]
                                 [--tree PATH --label NAME --kv-dtypes bf16]

kernel   evo_attn_decode_fp8 beside evo_attn_decode_bf16 on the same shapes (1 x 8k, 3 x 8k, 1 x 32k, 1 x 131k, 32 x 8k keys at H = 32), by
         device events: microseconds and the achieved TB/s of the bytes each form actually reads (K, V and, for FP8, the scales).
append   the fused rotary + append launch beside its bf16 sibling at 8 and 32 rows.
pool     DecodePool, --slots slots, evo-1-8k dimensions, synthetic weights, prompts of --prompt-len nt, one sample each, --tokens tokens:
         tokens / s over the whole job, the median device time of a captured step, stats["kv_bytes"], for kv_dtype bf16 and fp8.
long     the same with ONE stream behind a --long-len prompt on evo-1-131k dimensions: ms per token.
quality  the trained-like weight set (synthetic profile "contractive"): last-position logits rel-L2 and greedy agreement over 96 tokens
         behind a --prompt-len prompt, FP8 against bf16 cache.
Every figure is the median of --runs timed repetitions after --warmup untimed ones, with (min, max) beside it.  One JSON line.
--tree PATH imports evo_amd from another checkout (with its own build of the library) instead of this one and --kv-dtypes bf16 restricts
the pool / long legs to the default cache: the parent commit's tree, which has no FP8 cache, run as a second process of the same call shows
that the default path is where it was."""
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
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--prompt-len", type=int, default=8192)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--long-len", type=int, default=131072)
    ap.add_argument("--long-tokens", type=int, default=32)
    ap.add_argument("--tree", default=None, help="import evo_amd from this checkout instead of the one the tool lives in")
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--kv-dtypes", default="bf16,fp8")
    ap.add_argument("--small", action="store_true", help="the 4-layer test model instead of the 7B dimensions (a rehearsal, not a measurement)")
    args = ap.parse_args(argv)
    legs = [x for x in args.legs.split(",") if x]
    kv_dtypes = [x for x in args.kv_dtypes.split(",") if x]
    sys.path.insert(0, os.path.abspath(args.tree) if args.tree else HERE)
    import numpy as np
    import torch
    import evo_amd
    from evo_amd import ops as evo_ops
    from evo_amd.pool import DecodePool
    from evo_amd.tokenizer import CharLevelTokenizer
    if not torch.cuda.is_available():
        raise SystemExit("bench_kv_fp8: needs the GPU (no CPU timing path)")
    dev = "cuda:0"
    tok = CharLevelTokenizer(512)
    ops = evo_ops.default_ops()
    out = {"tree": args.label, "evo_amd": os.path.relpath(os.path.dirname(os.path.abspath(evo_amd.__file__))), "runs": args.runs, "warmup": args.warmup}
    if "kernel" in legs or "append" in legs:
        from evo_amd.sh.cache import Fp8KV

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
    if "kernel" in legs:
        out["kernel"] = []
        for B, n in ((1, 8192), (3, 8192), (1, 32768), (1, 131072), (32, 8192)):
            g = torch.Generator(device=dev).manual_seed(n + B)
            q = torch.randn(B, 1, H, 128, generator=g, device=dev).bfloat16()
            kv = torch.randn(B, n, 2, H, 128, generator=g, device=dev).bfloat16()
            f8 = Fp8KV.zeros(B, n, H, 128, dev)
            ops.kv_quant_fp8(kv[:, :, 0], kv[:, :, 1], f8, t0=0)
            pos = torch.full((B,), n - 1, dtype=torch.int64, device=dev)
            fns = {"bf16": lambda: ops.attention_decode(q, kv[:, :, 0], kv[:, :, 1], pos=pos),
                   "fp8": lambda: ops.attention_decode_fp8(q, f8, pos=pos),
                   "fp8_64_splits": lambda: ops.attention_decode_fp8(q, f8, pos=pos, n_splits=64)}     # (twice the default's waves: information only)
            diff = (fns["fp8"]().float() - fns["bf16"]().float()).norm() / fns["bf16"]().float().norm()
            t = alternate(fns, 20 if B * n <= 65536 else 8)
            need = {"bf16": B * n * 2 * H * 128 * 2, "fp8": B * n * 2 * H * (128 + 4)}
            need["fp8_64_splits"] = need["fp8"]
            out["kernel"].append({"B": B, "keys": n, "H": H, "rel_l2_fp8_vs_bf16": round(float(diff), 5), "bytes_read": need,
                                  **{k + "_us": med([1e3 * x for x in v]) for k, v in t.items()},
                                  **{k + "_TBs": round(need[k] / (statistics.median(t[k]) * 1e-3) / 1e12, 3) for k in t},
                                  "fp8_over_bf16_time": round(statistics.median(t["fp8"]) / statistics.median(t["bf16"]), 3)})
            del q, kv, f8
            torch.cuda.empty_cache()

    if "append" in legs:
        out["append"] = []
        inv = (1.0 / (10000.0 ** (torch.arange(0, 128, 2, dtype=torch.float32, device=dev) / 128))).contiguous()
        for B in (8, 32):
            cap = 8192
            g = torch.Generator(device=dev).manual_seed(B)
            qkv = torch.randn(B, 1, 3, H, 128, generator=g, device=dev).bfloat16()
            kv = torch.zeros(B, cap, 2, H, 128, dtype=torch.bfloat16, device=dev)
            f8 = Fp8KV.zeros(B, cap, H, 128, dev)
            pos = torch.randint(0, cap, (B,), generator=g, device=dev)
            a, b = qkv.clone(), qkv.clone()
            fns = {"bf16": lambda: ops.rope_append_decode(a, kv, pos, inv, 1.0, q_scale=ops.attn_q_scale(128)),
                   "fp8": lambda: ops.rope_append_decode_fp8(b, f8, pos, inv, 1.0, q_scale=ops.attn_q_scale(128))}
            t = alternate(fns, 200)
            out["append"].append({"rows": B, "H": H, **{k + "_us": med([1e3 * x for x in v]) for k, v in t.items()}})

    def model_of(name, profile="default"):
        if args.small:
            from evo_amd.sh.model import StripedHyena
            from evo_amd.synthetic import synthetic_state_dict
            cfg = dict(vocab_size=512, hidden_size=512, num_layers=4, attn_layer_idxs=[1], num_attention_heads=4)
            if "131k" in name:
                cfg.update(use_interpolated_rotary_pos_emb=True, rotary_emb_scaling_factor=16)
            m = StripedHyena(cfg)
            m.load_state_dict(synthetic_state_dict(m, seed=0), strict=True)
            m.to_bfloat16_except_poles_residues()
            return m.to(dev).eval()
        if profile == "default":
            return evo_amd.Evo(name, device=dev, weights="synthetic").model.eval()
        from evo_amd.models import _CONFIG_FOR, load_config
        from evo_amd.sh.model import StripedHyena
        from evo_amd.synthetic import synthetic_state_dict
        m = StripedHyena(load_config(_CONFIG_FOR[name]))
        m.load_state_dict(synthetic_state_dict(m, seed=0, device=dev, profile=profile), strict=True)
        m.to_bfloat16_except_poles_residues()
        return m.to(dev).eval()

    def pool_leg(model, n_slots, prompts, n_tokens):
        res = {kd: {"s": [], "step_ms": [], "kv_bytes": None} for kd in kv_dtypes}
        for it in range(args.warmup + args.runs):
            for kd in kv_dtypes:
                gc.collect()
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                pool = DecodePool(model, tok, n_slots=n_slots, top_k=4, top_p=1.0, temperature=0.7, device=dev, use_graph=True, seed=it,
                                  **({} if kd == "bf16" else {"kv_dtype": kd}))
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
                    res[kd]["s"].append(dt)
                    res[kd]["step_ms"].append(statistics.median(a.elapsed_time(b) for a, b in marks[2:]))     # (steps 0, 1: eager, capture)
                    res[kd]["kv_bytes"] = pool.stats.get("kv_bytes", sum(t.numel() * t.element_size() for t in
                                                                         pool.ipd["mha"].key_value_memory_dict.values()
                                                                         if isinstance(t, torch.Tensor)))
                pool._step_sampled = step = None
                del pool, marks
        n_gen = len(prompts) * n_tokens
        return {kd: {"tokens_per_s": round(n_gen / statistics.median(r["s"]), 1), "job_s": med(r["s"], 3), "step_ms": med(r["step_ms"], 4),
                     "kv_bytes": r["kv_bytes"]} for kd, r in res.items()}

    rng = np.random.default_rng(0)
    if "pool" in legs:
        model = model_of("evo-1-8k-base")
        prompts = ["".join(rng.choice(list("ACGT"), size=args.prompt_len)) for _ in range(args.slots)]
        out["pool"] = {"slots": args.slots, "prompt_len": args.prompt_len, "tokens": args.tokens, **pool_leg(model, args.slots, prompts, args.tokens)}
        del model
    if "long" in legs:
        model = model_of("evo-1-131k-base")
        prompts = ["".join(rng.choice(list("ACGT"), size=args.long_len))]
        out["long"] = {"slots": 1, "prompt_len": args.long_len, "tokens": args.long_tokens, **pool_leg(model, 1, prompts, args.long_tokens)}
        del model
    if "quality" in legs:
        from evo_amd.generation import Generator
        model = model_of("evo-1-8k-base", profile="contractive")
        prompt = "".join(rng.choice(list("ACGT"), size=args.prompt_len))
        got = {}
        for kd in ("bf16", "fp8"):
            ids, logits, _ = Generator(model, tok, top_k=1, kv_dtype=kd).generate(dev, input_string=prompt, num_tokens=96, print_generation=False)
            got[kd] = (ids[0].cpu(), logits[0].double().cpu())
        same = (got["fp8"][0] == got["bf16"][0]).long().cumprod(0)
        n = min(int(same.sum()) + 1, 96)
        a, b = got["fp8"][1], got["bf16"][1]
        out["quality"] = {"weights": "synthetic, profile contractive", "prompt_len": args.prompt_len, "greedy_tokens": 96,
                          "first_step_rel_l2": float((a[0] - b[0]).norm() / b[0].norm()),
                          "common_prefix_steps": n, "common_prefix_rel_l2": float((a[:n] - b[:n]).norm() / b[:n].norm()),
                          "tokens_agreeing": int((got["fp8"][0] == got["bf16"][0]).sum())}
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
