#!/usr/bin/env python
"""Embedding cost against the scoring forward, on evo-1-8k-base-sized synthetic weights: one JSON line.

Timed in one process, after warm-up, with device events around every call and a synchronise: the scoring forward (hidden_states + the
fused unembed / log-softmax / gather tail: what score_sequences runs), embeddings(layers=[15]) and embeddings(layers=["final"]), both
mean-pooled, at 8 x 8,192 and 1 x 131,072 nucleotides (+ BOS).  Also the pooling kernel alone on the final stream (fused norm) and its
algorithmic bytes: the pooled rows, read once.  The kernel's own time comes from a separate `rocprofv3 --kernel-trace --stats` run.

    python tools/bench_embed.py [--steps 5] [--warmup 2] [--only 8k|131k]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402


def build_model(name, device, seed=0):
    from evo_amd.models import _CONFIG_FOR, load_config
    from evo_amd.sh.model import StripedHyena
    from evo_amd.synthetic import synthetic_state_dict
    m = StripedHyena(load_config(_CONFIG_FOR[name]))
    m.load_state_dict(synthetic_state_dict(m, seed=seed, device=device), strict=True)
    m.to_bfloat16_except_poles_residues()
    return m.to(device)


def acgt_ids(batch, nt, seed0, device):
    rows = [np.random.default_rng(seed0 + b).choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=nt) for b in range(batch)]
    ids = np.concatenate([np.zeros((batch, 1), np.int64), np.stack(rows).astype(np.int64)], axis=1)
    return torch.from_numpy(ids).to(device)


def timed_ms(fn, steps, warmup):
    """Median of `steps` device-event timings of fn (after `warmup` calls), each ended by a synchronise."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(steps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), [round(t, 3) for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", choices=["8k", "131k"], default=None)
    args = ap.parse_args()
    from evo_amd.scoring import score_logprobs_device
    dev = "cuda:0"
    out = {"metric": "embedding forward vs scoring forward, evo-1 7B synthetic weights", "unit": "ms (median of device-event timings)",
           "steps": args.steps, "warmup": args.warmup, "shapes": {}}
    shapes = [("8x8192", "evo-1-8k-base", 8, 8192), ("1x131072", "evo-1-131k-base", 1, 131072)]
    for key, name, B, nt in shapes:
        if args.only and not key.endswith(args.only):
            continue
        model = build_model(name, dev)
        ids = acgt_ids(B, nt, 1234, dev)
        T = nt + 1
        D = model.hidden_size
        r = {}
        with torch.inference_mode():
            r["scoring_forward_ms"], r["scoring_samples"] = timed_ms(lambda: score_logprobs_device(model, ids), args.steps, args.warmup)
            r["embed_layer15_mean_ms"], r["embed_layer15_samples"] = timed_ms(lambda: model.embeddings(ids, [15]), args.steps, args.warmup)
            r["embed_final_mean_ms"], r["embed_final_samples"] = timed_ms(lambda: model.embeddings(ids, ["final"]), args.steps, args.warmup)
            # the pooling kernel alone, on a stream of the same shape (fused norm, mean over positions 1 .. T - 1 of every row)
            h = model.hidden_states(ids)
            ranges = [(b * T + 1, T - 1) for b in range(B)]
            r["pool_kernel_event_ms"], _ = timed_ms(lambda: model.ops.pool_rows(h, ranges, scale=model.norm.scale, eps=model.eps),
                                                    max(args.steps, 10), args.warmup)
            del h
        r["pool_bytes"] = B * (T - 1) * D * 2
        r["pool_event_TBps"] = r["pool_bytes"] / (r["pool_kernel_event_ms"] * 1e-3) / 1e12
        r["layer15_over_scoring"] = r["embed_layer15_mean_ms"] / r["scoring_forward_ms"]
        r["final_over_scoring"] = r["embed_final_mean_ms"] / r["scoring_forward_ms"]
        r["pool_share_of_final_embed"] = r["pool_kernel_event_ms"] / r["embed_final_mean_ms"]
        out["shapes"][key] = r
        del model
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
