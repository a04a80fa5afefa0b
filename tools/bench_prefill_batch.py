#!/usr/bin/env python
"""Times the decode pool with batched (ragged) prefill against the pool that prefills every prompt alone, in one process (not part of
bench.py), and the per-row end-state launch beside the Hyena operator's own launch on the same z^T.

    python tools/bench_prefill_batch.py [--slots 32] [--prompts 16] [--samples 4] [--tokens 128] [--batch 8] [--runs 3] [--warmup 1]
                                        [--small] [--no-pool] [--no-kernel]

Pool leg: bench.py's pool mix -- 7B synthetic weights (--small: the 4-layer test model), 16 prompts of 512-1,024 nt x 4 samples, 32
slots, 128 tokens each, the host sampler.  prefill_batch = 1 (the parent code path) and --batch alternate; the median of --runs timed
runs after --warmup untimed ones: generated tokens / s over the whole job (prefills included) and the device time between the first
and the last launch of every prefill (events), summed over the job.
Kernel leg: one evo_hyena_state_at_zt call (both launches) beside one evo_hyena_ct call (y, no state) on the same z^T at 8 x 1,024 and
1 x 8,192, D = 4,096 -- with every row at its full length (the most the state launch can cost) and, at 8 x 1,024, with lengths spread
over 512-1,024; alternating, the median of --runs x 20 calls.  One JSON line, with the box's own rates beside it."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", type=int, default=32)
    ap.add_argument("--prompts", type=int, default=16)
    ap.add_argument("--samples", type=int, default=4)
    ap.add_argument("--tokens", type=int, default=128)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--no-pool", action="store_true")
    ap.add_argument("--no-kernel", action="store_true")
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    import evo_amd
    from evo_amd import ops as evo_ops
    from evo_amd.pool import DecodePool
    from evo_amd.tokenizer import CharLevelTokenizer
    if not torch.cuda.is_available():
        raise SystemExit("bench_prefill_batch: no GPU -- nothing is measured without one")
    dev = "cuda:0"
    ops = evo_ops.default_ops()
    out = {"runs": args.runs, "warmup": args.warmup}

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
        from evo_amd.hyena_tables import mfma_operand_table
        D, H = (256, 2) if args.small else (4096, 32)
        g = torch.Generator(device=dev).manual_seed(1)
        fir_w = (torch.randn(3 * D, 3, generator=g, device=dev) * 0.3).bfloat16()
        fir_b = (torch.randn(3 * D, generator=g, device=dev) * 0.1).bfloat16()
        one_minus = 10.0 ** (-5.0 + 4.0 * torch.rand(D, 8, device=dev, generator=g))
        ang = (torch.rand(D, 8, device=dev, generator=g) * 2 - 1) * 3.141592653589793
        poles = torch.stack([(1 - one_minus) * torch.cos(ang), (1 - one_minus) * torch.sin(ang)], -1).float().contiguous()
        res = (torch.randn(D, 8, 2, device=dev, generator=g) * torch.sqrt(one_minus).unsqueeze(-1)).float().contiguous()
        dskip = (torch.randn(D, generator=g, device=dev) * 0.5).bfloat16()
        table = mfma_operand_table(poles, res, dskip)
        out["kernel"] = []
        for B, T in ((8, 1024), (1, 8192)):
            zt = ops.zt_from_rows(torch.randn(B, T, 3 * D, generator=g, device=dev).bfloat16(), B, T)
            yb = ops.yblk_empty(B * T, D, dev)
            full = torch.full((B,), T, dtype=torch.int64, device=dev)
            spread = torch.linspace(T // 2, T, B, device=dev).to(torch.int64)
            legs = {"hyena_ct": lambda: ops.hyena_ct(zt, B, T, fir_w, fir_b, table, H, y_blk=yb),
                    "hyena_ct_with_state": lambda: ops.hyena_ct(zt, B, T, fir_w, fir_b, table, H, y_blk=yb, want_state=True, poles=poles),
                    "state_at_full": lambda: ops.hyena_state_at_zt(zt, B, T, full, fir_w, fir_b, poles, H)}
            if B > 1:
                legs["state_at_spread"] = lambda: ops.hyena_state_at_zt(zt, B, T, spread, fir_w, fir_b, poles, H)
            tk = {k: [] for k in legs}
            for it in range(args.warmup + args.runs):
                for name, fn in legs.items():
                    ms = ev_ms(fn, 20)
                    if it >= args.warmup:
                        tk[name].append(ms)
            s_ct = ops.hyena_ct(zt, B, T, fir_w, fir_b, table, H, y_blk=yb, want_state=True, poles=poles)[1]
            s_at = ops.hyena_state_at_zt(zt, B, T, full, fir_w, fir_b, poles, H)[0]
            read = B * T * 2 * D * 2                                   # the x1 | v thirds of z^T
            out["kernel"].append({"B": B, "T": T, "D": D, **{k + "_us": round(1e3 * statistics.median(v), 2) for k, v in tk.items()},
                                  "state_at_full_needed_GBs": round(read / (statistics.median(tk["state_at_full"]) * 1e-3) / 1e9, 1),
                                  "state_max_diff_vs_ct_over_max": float((s_at - s_ct).abs().max() / s_ct.abs().max())})
            del zt, yb

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
        tok = CharLevelTokenizer(512)
        rng = np.random.default_rng(4242)
        prompts = ["".join(rng.choice(list("ACGT"), size=int(n))) for n in rng.integers(512, 1025, size=args.prompts)]
        res = {1: {"s": [], "prefill_ms": []}, args.batch: {"s": [], "prefill_ms": []}}
        stats = {}
        for it in range(args.warmup + args.runs):
            for pb in (1, args.batch):
                pool = DecodePool(model, tok, n_slots=args.slots, top_k=4, top_p=1.0, temperature=0.7, device=dev, prefill_batch=pb)
                marks = []

                def timed(fn):
                    def run(*a, **kw):
                        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                        e0.record()
                        r = fn(*a, **kw)
                        e1.record()
                        marks.append((e0, e1))
                        return r
                    return run
                pool._prefill, pool._prefill_ragged = timed(pool._prefill), timed(pool._prefill_ragged)
                torch.manual_seed(0)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                seqs, _, _ = pool.generate(prompts, n_tokens=args.tokens, n_sample_per_prompt=args.samples)
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if it >= args.warmup:
                    res[pb]["s"].append(dt)
                    res[pb]["prefill_ms"].append(sum(a.elapsed_time(b) for a, b in marks))
                stats[pb] = dict(pool.stats)
                pool._prefill = pool._prefill_ragged = None
                if hasattr(model, "release_decode_graph"):
                    model.release_decode_graph()
                del pool, marks
        n_gen = len(prompts) * args.samples * args.tokens
        out["pool"] = {"slots": args.slots, "prompts": args.prompts, "samples": args.samples, "tokens": args.tokens,
                       "prompt_nt": [min(map(len, prompts)), max(map(len, prompts))], "model": "small" if args.small else "7B synthetic"}
        for pb, r in res.items():
            out["pool"][f"prefill_batch_{pb}"] = {"tokens_per_s": round(n_gen / statistics.median(r["s"]), 1),
                                                  "job_s": [round(x, 4) for x in r["s"]],
                                                  "prefill_ms": [round(x, 2) for x in r["prefill_ms"]], "stats": stats[pb]}

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
