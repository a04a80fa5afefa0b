#!/usr/bin/env python
"""Times evo_amd.score_variants against naive score_sequences on the same variants, in one process (not part of bench.py).

    python tools/bench_variants.py [--ref-len 8192] [--variants 96] [--runs 5] [--warmup 2] [--small]

7B synthetic weights (--small: the 4-layer test model), a random reference and evenly spread single substitutions.  The legs
alternate; the median of --runs timed runs after --warmup untimed ones is reported, with the token-count ratio from `stats` (the
ceiling of the speed-up).  Also times HipOps.attention_prefix against the shipped entry on replicated K / V (B = 8, P = 4,096,
Tq = 4,097).  One JSON line."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref-len", type=int, default=8192)
    ap.add_argument("--variants", type=int, default=96)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--checkpoint-every", type=int, default=512)
    ap.add_argument("--batch", type=int, default=8, help="sequences per naive score_sequences call")
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args(argv)
    import numpy as np
    import torch
    import evo_amd
    from evo_amd.tokenizer import CharLevelTokenizer
    dev = "cuda:0"
    tok = CharLevelTokenizer(512)
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
    rng = np.random.default_rng(0)
    ref = "".join(rng.choice(list("ACGT"), size=args.ref_len))
    sites = np.linspace(0, args.ref_len - 1, args.variants).astype(int)
    variants = [ref[:i] + ("A" if ref[i] != "A" else "C") + ref[i + 1:] for i in sites]

    def cached():
        return evo_amd.score_variants(ref, variants, model, tok, reduce_method="sum", checkpoint_every=args.checkpoint_every, device=dev)

    def naive():
        out = []
        for i in range(0, len(variants), args.batch):
            out += evo_amd.score_sequences(variants[i:i + args.batch], model, tok, reduce_method="sum", device=dev)
        return out

    t = {"cached": [], "naive": []}
    stats = None
    for it in range(args.warmup + args.runs):
        for name, fn in (("cached", cached), ("naive", naive)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            r = fn()
            torch.cuda.synchronize()
            if it >= args.warmup:
                t[name].append(time.perf_counter() - t0)
            if name == "cached":
                stats = r.stats
    ops = model.ops
    B, H, P, Tq = 8, 32, 4096, 4097
    g = torch.Generator(device=dev).manual_seed(1)
    kv = torch.randn(1, P, 2, H, 128, generator=g, device=dev).bfloat16()
    qkv = torch.randn(B, Tq, 3, H, 128, generator=g, device=dev).bfloat16()
    kc = torch.cat([kv[:, :, 0].expand(B, -1, -1, -1), qkv[:, :, 1]], 1).contiguous()
    vc = torch.cat([kv[:, :, 1].expand(B, -1, -1, -1), qkv[:, :, 2]], 1).contiguous()
    plane = ops.attention_prefix_vt(kv[0, :, 1])
    legs = {"prefix": lambda: ops.attention_prefix(qkv[:, :, 0], qkv[:, :, 1], qkv[:, :, 2], kv[0, :, 0], None, vt_pre=plane),
            "replicated": lambda: ops.attention(qkv[:, :, 0], kc, vc, P)}
    ta = {k: [] for k in legs}
    for it in range(args.warmup + args.runs):
        for name, fn in legs.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            if it >= args.warmup:
                ta[name].append(a.elapsed_time(b))
    # the box's own rates beside the figures (bench.py's `box` block: the HBM copy probe and the library GEMM)
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
    n = 1 << 30
    src = torch.empty(n, dtype=torch.uint8, device=dev).random_(0, 256)
    dst = torch.empty_like(src)
    st = torch.cuda.current_stream().cuda_stream
    copy_gbs = 2.0 * n / (ev_ms(lambda: ops.lib.evo_probe_copy_f4(src.data_ptr(), dst.data_ptr(), n, st), 20) * 1e-3) / 1e9
    del src, dst
    a_ = torch.randn(8192, 8192, generator=g, device=dev).bfloat16()
    b_ = torch.randn(8192, 8192, generator=g, device=dev).bfloat16()
    gemm_tflops = 2.0 * 8192 ** 3 / (ev_ms(lambda: torch.mm(a_, b_), 10) * 1e-3) / 1e12
    print(json.dumps({"box": {"hbm_copy_GBs": round(copy_gbs, 1), "library_gemm_tflops": round(gemm_tflops, 1)}, "ref_len": args.ref_len, "variants": args.variants, "runs": args.runs,
                      "score_variants_s": statistics.median(t["cached"]), "naive_s": statistics.median(t["naive"]),
                      "token_ratio": stats["naive_tokens"] / stats["tokens"], "stats": stats,
                      "attention_prefix_ms": statistics.median(ta["prefix"]), "attention_replicated_ms": statistics.median(ta["replicated"]),
                      "prefix_kv_bytes": int(kv.numel() * 2 + plane.numel() * 2), "replicated_prefix_kv_bytes": int(B * (kv.numel() * 2 + plane.numel() * 2))}))


if __name__ == "__main__":
    main()
