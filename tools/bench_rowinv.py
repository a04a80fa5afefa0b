#!/usr/bin/env python
"""Times the decode pool's batch-invariant step against the default step, legs alternated in one process (not part of bench.py; DESIGN.md
section 25).

    python tools/bench_rowinv.py [--legs launch,pool] [--runs 3] [--warmup 1] [--slots 1,4,8,16,32] [--prompt-len 8192] [--tokens 32]
                                 [--small] [--tree PATH --label NAME --modes default]

launch   the five dense launches of a 7B block and of the unembedding -- projections 12288 x 4096, out 4096 x 4096, gate 22016 x 4096,
         l3 4096 x 11008, unembedding 512 x 4096 -- at M = 1, 8 and 32 rows: the row-invariant entry beside what `ops` routes by default
         (for the two launches the default fuses a norm into, the default leg is the fused call and the invariant leg norm + launch);
         device events, microseconds.
pool     DecodePool at every slot count of --slots, evo-1-8k dimensions, synthetic weights, ONE prompt of --prompt-len nt sampled once per
         slot (one prefill per pool), --tokens tokens: the median device time of a captured step, option off and on alternated.
Every figure is the median of --runs timed repetitions after --warmup untimed ones, with (min, max) beside it.  One JSON line, with the
HBM copy probe of the run.  --tree PATH imports evo_amd from another checkout (with its own build of the library) and --modes default
restricts the legs to the default step: the parent commit's tree, which has no such option, run as a second process of the same call."""
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
    ap.add_argument("--legs", default="launch,pool")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--slots", default="1,4,8,16,32")
    ap.add_argument("--prompt-len", type=int, default=8192)
    ap.add_argument("--tokens", type=int, default=32)
    ap.add_argument("--tree", default=None, help="import evo_amd from this checkout instead of the one the tool lives in")
    ap.add_argument("--label", default="this tree")
    ap.add_argument("--modes", default="default,invariant")
    ap.add_argument("--small", action="store_true", help="the 4-layer test model instead of the 7B dimensions (a rehearsal, not a measurement)")
    args = ap.parse_args(argv)
    legs = [x for x in args.legs.split(",") if x]
    modes = [x for x in args.modes.split(",") if x]
    sys.path.insert(0, os.path.abspath(args.tree) if args.tree else HERE)
    import numpy as np
    import torch
    import evo_amd
    from evo_amd import ops as evo_ops
    from evo_amd.pool import DecodePool
    from evo_amd.tokenizer import CharLevelTokenizer
    if not torch.cuda.is_available():
        raise SystemExit("bench_rowinv: needs the GPU (no CPU timing path)")
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

    if "launch" in legs:
        out["launch"] = []
        D, I, V = (512, 1536, 512) if args.small else (4096, 11008, 512)
        g = torch.Generator(device=dev).manual_seed(0)

        def rnd(*shape, scale=1.0):
            return (torch.randn(*shape, generator=g, device=dev) * scale).bfloat16()
        scale_v = rnd(D).abs() + 0.5
        w_in, b_in, w_out, b_out = rnd(3 * D, D, scale=D ** -0.5), rnd(3 * D), rnd(D, D, scale=D ** -0.5), rnd(D)
        w12, w3, w_un = rnd(2 * I, D, scale=D ** -0.5), rnd(D, I, scale=I ** -0.5), rnd(V, D, scale=D ** -0.5)
        for M in (1, 8, 32):
            x, a, res = rnd(M, D), rnd(M, I), rnd(M, D)
            classes = {
                "norm+projection": {"default": lambda: ops.norm_linear(x, scale_v, 1e-6, w_in, b_in),
                                    "invariant": lambda: ops.linear_rowinv(ops.rmsnorm(x, None, scale_v, 1e-6), w_in, b_in)},
                "out+residual": {"default": lambda: ops.linear_residual_(res, x, w_out, bias=b_out),
                                 "invariant": lambda: ops.linear_residual_rowinv_(res, x, w_out, bias=b_out)},
                "norm+gate": {"default": lambda: ops.mlp_gate(x, w12, scale_v, 1e-6),
                              "invariant": lambda: ops.mlp_gate_rowinv(ops.rmsnorm(x, None, scale_v, 1e-6), w12)},
                "l3+residual": {"default": lambda: ops.linear_residual_(res, a, w3),
                                "invariant": lambda: ops.linear_residual_rowinv_(res, a, w3)},
                "unembedding": {"default": lambda: ops.linear(x, w_un, None),
                                "invariant": lambda: ops.linear_rowinv(x, w_un, None)},
            }
            row = {"M": M}
            for name, fns in classes.items():
                t = alternate({k: v for k, v in fns.items() if k in modes}, 50)
                row[name] = {k + "_us": med([1e3 * x_ for x_ in v]) for k, v in t.items()}
                if len(t) == 2:
                    row[name]["invariant_over_default"] = round(statistics.median(t["invariant"]) / statistics.median(t["default"]), 3)
            out["launch"].append(row)

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

    def pool_leg(model, n_slots, prompt, n_tokens):
        res = {mode: [] for mode in modes}
        for it in range(args.warmup + args.runs):
            for mode in modes:
                gc.collect()
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                pool = DecodePool(model, tok, n_slots=n_slots, top_k=4, top_p=1.0, temperature=0.7, device=dev, use_graph=True, seed=it,
                                  **({"batch_invariant": True} if mode == "invariant" else {}))
                marks, step = [], pool._step_sampled

                def timed_step():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    step()
                    e1.record()
                    marks.append((e0, e1))
                pool._step_sampled = timed_step
                pool.generate([prompt], n_tokens=n_tokens, n_sample_per_prompt=n_slots)
                torch.cuda.synchronize()
                if it >= args.warmup:
                    res[mode].append(statistics.median(a.elapsed_time(b) for a, b in marks[2:]))     # (steps 0, 1: eager, capture)
                pool._step_sampled = step = None
                del pool, marks
        row = {"slots": n_slots, **{mode + "_step_ms": med(v, 4) for mode, v in res.items()}}
        if len(res) == 2:
            row["invariant_over_default"] = round(statistics.median(res["invariant"]) / statistics.median(res["default"]), 3)
        return row

    if "pool" in legs:
        model = model_of("evo-1-8k-base")
        prompt = "".join(np.random.default_rng(0).choice(list("ACGT"), size=args.prompt_len))
        out["pool"] = {"prompt_len": args.prompt_len, "tokens": args.tokens,
                       "steps": [pool_leg(model, int(s), prompt, args.tokens) for s in args.slots.split(",") if s]}
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
