#!/usr/bin/env python
"""Times the FP8 (e4m3fn) decode weights against the bf16 weights, legs alternated in one process (not part of bench.py; DESIGN.md sections 22 and 28).

    python tools/bench_w8.py [--legs kernel,step,quality] [--runs 5] [--warmup 2] [--streams 1,4,8] [--rows 1,4,8] [--prompt-len 8192]
                             [--tokens 64] [--quality-streams 1] [--small] [--tree PATH --label NAME --weight-dtypes bf16]

kernel   every launch class of a 7B decode step at the M of --rows (1-64), FP8 beside bf16 on the same values: microseconds (device
         events) and the achieved TB/s of the weight bytes each form reads (FP8: bytes + 4 per row).  Above 8 rows neither format folds
         the norm or the Hyena step into the dense launch: the classes are then timed as the dense launches alone.
step     DecodePool, evo-1-8k dimensions, synthetic weights, --streams slots behind prompts of --prompt-len nt, --tokens tokens: the median
         device time of a captured step and stats["decode_weight_bytes"], for weight_dtype bf16 and fp8.
quality  the trained-like weight set (synthetic profile "contractive") at 7B width: last-position logits rel-L2 and greedy agreement over
         96 tokens behind --quality-streams prompts of --prompt-len nt in one batch, FP8 against bf16 weights (and, with --small, the
         toy model).
Every figure is the median of --runs timed repetitions after --warmup untimed ones, with (min, max) beside it.  One JSON line, the box's
copy probe beside the figures.  --tree PATH imports evo_amd from another checkout (with its own build of the library) and --weight-dtypes
bf16 restricts the legs to the default weights: the parent commit's tree run the same way shows that the default path is where it was."""
import argparse
import gc
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def med(v, digits=2):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--legs", default="kernel,step")
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--streams", default="1,4,8", help="pool sizes of the step leg, 1-64")
    ap.add_argument("--rows", default="1,4,8", help="batch rows of the kernel leg, 1-64")
    ap.add_argument("--quality-streams", type=int, default=1, help="prompts in the quality leg's batch, 1-64")
    ap.add_argument("--prompt-len", type=int, default=8192)
    ap.add_argument("--tokens", type=int, default=64)
    ap.add_argument("--tree", default=None, help="import evo_amd from this checkout instead of the one the tool lives in")
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--weight-dtypes", default="bf16,fp8")
    ap.add_argument("--small", action="store_true", help="the 4-layer test model instead of the 7B dimensions (a rehearsal, not a measurement)")
    args = ap.parse_args(argv)
    legs = [x for x in args.legs.split(",") if x]
    fmts = [x for x in args.weight_dtypes.split(",") if x]
    sys.path.insert(0, os.path.abspath(args.tree) if args.tree else HERE)
    import numpy as np
    import torch
    import evo_amd
    from evo_amd import ops as evo_ops
    from evo_amd.pool import DecodePool
    from evo_amd.tokenizer import CharLevelTokenizer
    if not torch.cuda.is_available():
        raise SystemExit("bench_w8: needs the GPU (no CPU timing path)")
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
        t = {k: [] for k in fns}
        for it in range(args.warmup + args.runs):
            for name, fn in fns.items():
                ms = ev_ms(fn, reps)
                if it >= args.warmup:
                    t[name].append(ms)
        return t

    def graph_of(calls):
        """One captured graph of the calls in order (a decode step runs captured: a launch then costs its 2 us, not the interpreter's)."""
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            calls[0]()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for c in calls:
                c()
        return g

    if "kernel" in legs:
        D, I, H = (512, 1536, 4) if args.small else (4096, 11008, 32)
        gen = torch.Generator(device=dev).manual_seed(0)
        scale = torch.ones(D, dtype=torch.bfloat16, device=dev)
        zb = torch.zeros(3 * D, dtype=torch.bfloat16, device=dev)
        fir_w = torch.zeros(3 * D, 3, dtype=torch.bfloat16, device=dev)
        poles, resd = torch.zeros(D, 8, 2, device=dev), torch.zeros(D, 8, 2, device=dev)
        out["kernel"] = []
        shapes = {"hyena_fused [3D, D]": (3 * D, D), "norm_linear Wqkv [3D, D]": (3 * D, D), "linear_residual out [D, D]": (D, D),
                  "norm_gate l1 | l2 [2I, D]": (2 * I, D), "linear_residual l3 [D, I]": (D, I)}
        for name, (N, K) in shapes.items():
            # as many copies of the weight as pass 1 GiB of FP8 bytes, walked in turn: no launch finds its weight in a cache
            copies = max(2, -(-(1 << 30) // (N * K)))
            ws = [(torch.randn(N, K, generator=gen, device=dev) / K ** 0.5).bfloat16() for _ in range(copies)]
            recs = [ops.w_quant_fp8(w) for w in ws] if "fp8" in fmts else [None] * copies
            for M in [int(r) for r in args.rows.split(",") if r]:
                x = torch.randn(M, K, generator=gen, device=dev).bfloat16()
                res = torch.zeros(M, D, dtype=torch.bfloat16, device=dev)
                fs = torch.zeros(M, 3 * D, 2, dtype=torch.bfloat16, device=dev)
                st = torch.zeros(M, D, 8, dtype=torch.complex64, device=dev)

                def call(fmt, w, rec):
                    if M > 8 and not name.startswith("linear_residual"):     # (no fold at these rows: the dense launch of the class)
                        if name.startswith("norm_gate"):
                            return (lambda: ops.mlp_gate(x, w)) if fmt == "bf16" else (lambda: ops.mlp_gate_w8(x, rec))
                        return (lambda: ops.linear(x, w, zb)) if fmt == "bf16" else (lambda: ops.linear_w8(x, rec, zb))
                    if name.startswith("hyena"):
                        if fmt == "bf16":
                            return lambda: ops.hyena_decode_fused(x, scale, 1e-6, w, zb, fs, st, fir_w, zb, poles, resd, zb[:D], H)
                        return lambda: ops.hyena_decode_fused_w8(x, scale, 1e-6, rec, zb, fs, st, fir_w, zb, poles, resd, zb[:D], H)
                    if name.startswith("norm_linear"):
                        return (lambda: ops.norm_linear(x, scale, 1e-6, w, zb)) if fmt == "bf16" else (lambda: ops.norm_linear_w8(x, scale, 1e-6, rec, zb))
                    if name.startswith("norm_gate"):
                        return (lambda: ops.mlp_gate(x, w, scale, 1e-6)) if fmt == "bf16" else (lambda: ops.mlp_gate_w8(x, rec, scale, 1e-6))
                    b = zb[:D] if "out" in name else None
                    return (lambda: ops.linear_residual_(res, x, w, bias=b)) if fmt == "bf16" else (lambda: ops.linear_residual_w8_(res, x, rec, bias=b))
                graphs = {f: graph_of([call(f, w, r) for w, r in zip(ws, recs)]) for f in fmts}
                t = alternate({f: g.replay for f, g in graphs.items()}, 3)
                t = {f: [v / copies for v in vs] for f, vs in t.items()}
                need = {"bf16": N * K * 2, "fp8": N * K + 4 * N}
                row = {"M": M, "class": name, "weight_copies": copies, **{k + "_us": med([1e3 * v for v in t[k]]) for k in t},
                       **{k + "_TBs": round(need[k] / (statistics.median(t[k]) * 1e-3) / 1e12, 3) for k in t}}
                if len(t) == 2:
                    row["fp8_over_bf16_time"] = round(statistics.median(t["fp8"]) / statistics.median(t["bf16"]), 3)
                out["kernel"].append(row)
                del graphs
            del ws, recs
            gc.collect()
            torch.cuda.empty_cache()

    def model_of(name, profile="default"):
        from evo_amd.sh.model import StripedHyena
        from evo_amd.synthetic import synthetic_state_dict
        if args.small:
            cfg = dict(vocab_size=512, hidden_size=512, num_layers=4, attn_layer_idxs=[1], num_attention_heads=4)
            m = StripedHyena(cfg)
            m.load_state_dict(synthetic_state_dict(m, seed=0), strict=True)
            m.to_bfloat16_except_poles_residues()
            return m.to(dev).eval()
        if profile == "default":
            return evo_amd.Evo(name, device=dev, weights="synthetic").model.eval()
        from evo_amd.models import _CONFIG_FOR, load_config
        m = StripedHyena(load_config(_CONFIG_FOR[name]))
        m.load_state_dict(synthetic_state_dict(m, seed=0, device=dev, profile=profile), strict=True)
        m.to_bfloat16_except_poles_residues()
        return m.to(dev).eval()

    rng = np.random.default_rng(0)
    if "step" in legs:
        model = model_of("evo-1-8k-base")
        out["step"] = []
        for S in [int(s) for s in args.streams.split(",") if s]:
            prompts = ["".join(rng.choice(list("ACGT"), size=args.prompt_len)) for _ in range(S)]
            res = {f: {"step_ms": [], "bytes": None} for f in fmts}
            for it in range(args.warmup + args.runs):
                for f in fmts:
                    gc.collect()
                    torch.cuda.synchronize()
                    pool = DecodePool(model, tok, n_slots=S, top_k=4, top_p=1.0, temperature=0.7, device=dev, use_graph=True, seed=it,
                                      **({} if f == "bf16" else {"weight_dtype": f}))
                    marks, step = [], pool._step_sampled

                    def timed_step():
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        step()
                        e1.record()
                        marks.append((e0, e1))
                    pool._step_sampled = timed_step
                    pool.generate(prompts, n_tokens=args.tokens, n_sample_per_prompt=1)
                    torch.cuda.synchronize()
                    if it >= args.warmup:
                        res[f]["step_ms"].append(statistics.median(a.elapsed_time(b) for a, b in marks[2:]))   # (steps 0, 1: eager, capture)
                        res[f]["bytes"] = pool.stats.get("decode_weight_bytes")
                    pool._step_sampled = step = None
                    del pool, marks
            row = {"streams": S, "prompt_len": args.prompt_len, "tokens": args.tokens,
                   **{f: {"step_ms": med(r["step_ms"], 4), "decode_weight_bytes": r["bytes"]} for f, r in res.items()}}
            if len(fmts) == 2:
                row["fp8_over_bf16_time"] = round(statistics.median(res["fp8"]["step_ms"]) / statistics.median(res["bf16"]["step_ms"]), 3)
            out["step"].append(row)
        del model
    if "quality" in legs:
        from evo_amd.generation import Generator
        model = model_of("evo-1-8k-base", profile="contractive")
        QS = args.quality_streams
        prompts = torch.tensor([list("".join(rng.choice(list("ACGT"), size=args.prompt_len)).encode()) for _ in range(QS)], device=dev)
        got = {}
        for f in ("bf16", "fp8"):
            ids, logits, _ = Generator(model, tok, top_k=1, weight_dtype=f).generate(dev, input_ids=prompts, num_tokens=96, print_generation=False,
                                                                                     stop_at_eos=False)
            got[f] = (ids[0].cpu(), logits[0].double().cpu(), logits[:, 1].double().cpu())
        same = (got["fp8"][0] == got["bf16"][0]).long().cumprod(0)
        n = min(int(same.sum()) + 1, 96)
        a, b = got["fp8"][1], got["bf16"][1]
        out["quality"] = {"weights": "toy, synthetic" if args.small else "synthetic, profile contractive", "prompt_len": args.prompt_len,
                          "streams": QS, "second_step_rel_l2_all_rows": float((got["fp8"][2] - got["bf16"][2]).norm() / got["bf16"][2].norm()),
                          "greedy_tokens": 96, "second_step_rel_l2": float((a[1] - b[1]).norm() / b[1].norm()),
                          "common_prefix_steps": n, "common_prefix_rel_l2": float((a[:n] - b[:n]).norm() / b[:n].norm()),
                          "tokens_agreeing": int((got["fp8"][0] == got["bf16"][0]).sum())}
        del model
    gc.collect()
    torch.cuda.empty_cache()
    n = 1 << 30
    src = torch.empty(n, dtype=torch.uint8, device=dev).random_(0, 256)
    dst = torch.empty_like(src)
    st = torch.cuda.current_stream().cuda_stream
    ev_ms(lambda: ops.lib.evo_probe_copy_f4(src.data_ptr(), dst.data_ptr(), n, st), 3)
    out["box"] = {"hbm_copy_GBs": round(2.0 * n / (ev_ms(lambda: ops.lib.evo_probe_copy_f4(src.data_ptr(), dst.data_ptr(), n, st), 20) * 1e-3) / 1e9, 1)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
