#!/usr/bin/env python
"""GB/s of the skinny dense layer (evo_linear_small_m_bf16) vs torch/hipBLASLt for the decode shapes.

`--fused`: instead, the launches that fold a norm, a gate or the Hyena step around the weight stream (csrc/gemv.hip), one
JSON line per (entry, M): evo_norm_linear_small_m_bf16 (N = 12288), evo_norm_mlp_gate_small_m_bf16 and evo_mlp_gate_small_m_bf16
(I = 11008, grouped) and evo_hyena_decode_fused_small_m (D = 4096, 32 heads), all at K = 4096.  Six weight copies in turn, captured as one
graph; the figure is the median over 7 blocks of 216 launches each, between device events.  EVO_AMD_LIBNAME picks the library: an A/B
comparison runs this once per process and library, alternating."""
import json
import math
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from evo_amd.ops import default_ops  # noqa: E402

ops = default_ops()
dev = "cuda:0"
g = torch.Generator(device=dev).manual_seed(0)
tag = os.environ.get("EVO_AMD_LIBNAME", "default")


def timeit(fn, n=20):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def fused_entries(M):
    """(entry, weight bytes, [one launch closure per weight copy]) for the four fused launches at M rows."""
    K = D = 4096
    I, H, COPIES = 11008, 32, 6
    rn = lambda *s, std=1.0: torch.randn(*s, generator=g, device=dev) * std  # noqa: E731
    x = rn(M, K).bfloat16()
    scale = rn(K, std=0.1).add_(1).bfloat16()
    w = [rn(12288, K, std=0.02).bfloat16() for _ in range(COPIES)]
    yield "evo_norm_linear_small_m_bf16", 12288 * K * 2, [lambda wi=wi: ops.norm_linear(x, scale, 1e-6, wi, None) for wi in w]
    del w
    w = [ops.pack_gate_weights(rn(2 * I, K, std=0.02).bfloat16()) for _ in range(COPIES)]
    yield "evo_norm_mlp_gate_small_m_bf16", 2 * I * K * 2, [lambda wi=wi: ops.mlp_gate(x, None, scale, 1e-6, w12g=wi) for wi in w]
    yield "evo_mlp_gate_small_m_bf16", 2 * I * K * 2, [lambda wi=wi: ops.mlp_gate(x, None, w12g=wi) for wi in w]
    del w
    sets = []
    for _ in range(COPIES):
        mag = 1 - 10 ** (-5 + 4 * torch.rand(D, 8, generator=g, device=dev))
        ang = (torch.rand(D, 8, generator=g, device=dev) * 2 - 1) * math.pi
        sets.append((scale, 1e-6, rn(3 * D, D, std=0.02).bfloat16(), rn(3 * D, std=0.1).bfloat16(), rn(M, 3 * D, 2).bfloat16(),
                     torch.view_as_complex(rn(M, D, 8, 2, std=0.5).float().contiguous()), rn(3 * D, 3, std=0.3).bfloat16(),
                     rn(3 * D, std=0.1).bfloat16(), torch.stack([mag * torch.cos(ang), mag * torch.sin(ang)], -1).float().contiguous(),
                     rn(D, 8, 2, std=0.25).float().contiguous(), rn(D, std=0.5).bfloat16(), H))
    yield "evo_hyena_decode_fused_small_m", 3 * D * D * 2, [lambda b=b: ops.hyena_decode_fused(x, *b) for b in sets]


def time_graph(fns, blocks=7, replays=36):
    """us per launch of the launches `fns`, captured in this order as one graph: the median over `blocks` of `replays` replays each."""
    for f in fns:
        f()
    torch.cuda.synchronize()
    gr, st = torch.cuda.CUDAGraph(), torch.cuda.Stream()
    with torch.cuda.stream(st):
        with torch.cuda.graph(gr):
            for f in fns:
                f()
    for _ in range(3):
        gr.replay()
    torch.cuda.synchronize()
    per = []
    for _ in range(blocks):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(replays):
            gr.replay()
        e1.record()
        torch.cuda.synchronize()
        per.append(e0.elapsed_time(e1) * 1e3 / (replays * len(fns)))
    return statistics.median(per), min(per), max(per)


if "--fused" in sys.argv[1:]:
    for M in [int(v) for v in os.environ.get("GEMV_MS", "1,2,4,8").split(",")]:
        for entry, nbytes, fns in fused_entries(M):
            med, lo, hi = time_graph(fns)
            print(json.dumps(dict(lib=tag, entry=entry, M=M, us=round(med, 3), us_min=round(lo, 3), us_max=round(hi, 3),
                                  launches=7 * 36 * len(fns), weight_TBps=round(nbytes / med / 1e6, 3))), flush=True)
    sys.exit(0)

for M in [int(x) for x in os.environ.get("GEMV_MS", "1,2,4,5,8,12,16,32,48,64").split(",")]:
    tot_mine = tot_torch = 0.0
    line = []
    for name, N, K in (("proj", 12288, 4096), ("out", 4096, 4096), ("l1l2", 22016, 4096), ("l3", 4096, 11008)):
        # rotate over several weight copies so the 256 MB Infinity Cache cannot hold the operand
        ws = [(torch.randn(N, K, generator=g, device=dev) * 0.02).bfloat16() for _ in range(6)]
        x = torch.randn(M, K, generator=g, device=dev).bfloat16()
        it = [0]

        def mine():
            it[0] = (it[0] + 1) % len(ws)
            return ops._linear_small_m(x, ws[it[0]], None, None)

        def ref():
            it[0] = (it[0] + 1) % len(ws)
            return torch.mm(x, ws[it[0]].t())

        a, b = timeit(mine), timeit(ref)
        tot_mine += a
        tot_torch += b
        line.append(f"{name} {N * K * 2 / a / 1e6:5.0f}/{N * K * 2 / b / 1e6:5.0f}")
        del ws
    print(f"[{tag}] M={M}: GB/s mine/torch: " + "  ".join(line) + f" | per block {tot_mine * 1e3:.0f} vs {tot_torch * 1e3:.0f} us")
