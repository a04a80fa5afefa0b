#!/usr/bin/env python
"""Times the beam-search step against the sampling step of the same pool shape, legs alternated in one process (not part of bench.py;
DESIGN.md section 24).

    python tools/bench_beam.py [--slots 8,32] [--widths 4,8] [--tokens 64,512] [--prompt-len 8192] [--runs 3] [--warmup 1] [--small]
                               [--budget-s SECONDS]

For every (slots, width, tokens): slots // width prompts of --prompt-len nt, 7B dimensions, synthetic weights, `share_prompt_kv=True`.
sampling   DecodePool.generate with `width` samples per prompt (the same slots, the same store rows): the captured sampling step.
beam       DecodePool.beam_search at that width: the captured step = forward + evo_beam_select_f32 + evo_gather_rows out and back.
Both report the median device time of a captured step (steps 0 and 1, eager and capture, left out), as the median of --runs repetitions
after --warmup untimed ones with (min, max) beside it, and beam / sampling.  `kernels`: on the state the last search left behind, the
selection launch alone and the two copy launches alone, under the worst parent map (every slot continues its neighbour: all rows move)
and under the identity (nothing moves).  The cases run in the order tokens, slots, width; every finished case is printed as a JSON line
of its own, then one JSON line holds them all with the HBM copy probe of the run.  --budget-s: a case is started only while the cases
so far took less than this; the others are listed under "not_run"."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def med(v, digits=4):
    return {"median": round(statistics.median(v), digits), "min": round(min(v), digits), "max": round(max(v), digits)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--slots", default="8,32")
    ap.add_argument("--widths", default="4,8")
    ap.add_argument("--tokens", default="64,512")
    ap.add_argument("--prompt-len", type=int, default=8192)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--budget-s", type=float, default=None)
    ap.add_argument("--small", action="store_true", help="the 4-layer test model instead of the 7B dimensions (a rehearsal, not a measurement)")
    args = ap.parse_args(argv)
    sys.path.insert(0, HERE)
    import numpy as np
    import torch
    import evo_amd
    from evo_amd import ops as evo_ops
    from evo_amd.pool import DecodePool
    from evo_amd.tokenizer import CharLevelTokenizer
    if not torch.cuda.is_available():
        raise SystemExit("bench_beam: needs the GPU (no CPU timing path)")
    dev = "cuda:0"
    tok = CharLevelTokenizer(512)
    ops = evo_ops.default_ops()
    if args.small:
        from evo_amd.sh.model import StripedHyena
        from evo_amd.synthetic import synthetic_state_dict
        m = StripedHyena(dict(vocab_size=512, hidden_size=512, num_layers=4, attn_layer_idxs=[1], num_attention_heads=4))
        m.load_state_dict(synthetic_state_dict(m, seed=0), strict=True)
        m.to_bfloat16_except_poles_residues()
        model = m.to(dev).eval()
    else:
        model = evo_amd.Evo("evo-1-8k-base", device=dev, weights="synthetic").model.eval()

    def ev_ms(fn, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / reps

    def timed(pool, name):
        """Wrap pool.<name> so that every call is bracketed by device events -> the list of (start, end) pairs."""
        marks, step = [], getattr(pool, name)

        def timed_step():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step()
            e1.record()
            marks.append((e0, e1))
        setattr(pool, name, timed_step)
        return marks

    rng = np.random.default_rng(0)
    out = {"prompt_len": args.prompt_len, "runs": args.runs, "warmup": args.warmup, "model": "toy" if args.small else "evo-1-8k-base (synthetic)",
           "cases": []}
    t_start = time.perf_counter()
    out["not_run"] = []
    shapes = [(S, W) for S in (int(x) for x in args.slots.split(",")) for W in (int(x) for x in args.widths.split(",")) if W <= S]
    prompts_of = {(S, W): ["".join(rng.choice(list("ACGT"), size=args.prompt_len)) for _ in range(S // W)] for S, W in shapes}
    for n_tokens in (int(x) for x in args.tokens.split(",")):
        for S, W in shapes:
            if True:
                prompts = prompts_of[(S, W)]
                if args.budget_s is not None and time.perf_counter() - t_start > args.budget_s:
                    out["not_run"].append({"slots": S, "width": W, "tokens": n_tokens})
                    continue
                t = {"sampling": [], "beam": []}
                last = None
                for it in range(args.warmup + args.runs):
                    for leg in ("sampling", "beam"):
                        gc.collect()
                        torch.cuda.synchronize()
                        torch.cuda.empty_cache()
                        pool = DecodePool(model, tok, n_slots=S, top_k=4, top_p=1.0, temperature=0.7, device=dev, use_graph=True, seed=it,
                                          allowed_tokens="ACGT", share_prompt_kv=True)
                        if leg == "sampling":
                            marks = timed(pool, "_step_sampled")
                            pool.generate(prompts, n_tokens=n_tokens, n_sample_per_prompt=W)
                        else:
                            marks = timed(pool, "_step_beam")
                            pool.beam_search(prompts, n_tokens, beam_width=W)
                            last = pool
                        torch.cuda.synchronize()
                        if it >= args.warmup:
                            t[leg].append(statistics.median(a.elapsed_time(b) for a, b in marks[2:]))
                        del marks
                        if leg == "sampling":
                            del pool
                case = {"slots": S, "width": W, "tokens": n_tokens, "sampling_step_ms": med(t["sampling"]), "beam_step_ms": med(t["beam"]),
                        "beam_over_sampling": round(statistics.median(t["beam"]) / statistics.median(t["sampling"]), 4),
                        "rows_moved": last.stats["beam_rows_moved"], "scratch_bytes": last.stats["beam_scratch_bytes"]}
                # the two kernels alone, on the state the search left: own_pos = n_tokens - 1 (every generated key is live)
                b = last._beam
                logits = torch.randn(S, 512, device=dev).bfloat16()
                b["cum"].zero_()
                b["ended"].zero_()
                b["active"].fill_(1)
                b["step"].zero_()
                sel = [ev_ms(lambda: last._beam_select(logits, b["active"]), 20) for _ in range(args.warmup + args.runs)][args.warmup:]
                own = last.store.own_pos
                shift = (torch.arange(S, device=dev) + 1) % S
                ident = torch.arange(S, device=dev)
                mv = [ev_ms(lambda: ops.gather_rows(b["table"], shift, own), 5) for _ in range(args.warmup + args.runs)][args.warmup:]
                idn = [ev_ms(lambda: ops.gather_rows(b["table"], ident, own), 20) for _ in range(args.warmup + args.runs)][args.warmup:]
                moved = sum(int(r[2]) if int(r[3]) == 0 else min(int(own.max()) + 1, int(r[2]) // int(r[3])) * int(r[3])
                            for r in b["table"].table.cpu().tolist()) * S
                case["kernels"] = {"beam_select_us": med([1e3 * x for x in sel], 2), "gather_all_rows_us": med([1e3 * x for x in mv], 2),
                                   "gather_identity_us": med([1e3 * x for x in idn], 2), "gather_all_rows_bytes_one_way": moved,
                                   "gather_all_rows_GBs": round(4.0 * moved / (statistics.median(mv) * 1e-3) / 1e9, 1)}
                out["cases"].append(case)
                print(json.dumps(case), flush=True)
                del last, pool, b
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
