#!/usr/bin/env python
"""FASTA -> .npz of sequence embeddings (companion of scripts/score.py: same model flags, sequences bucketed by length before batching).

    python -m scripts.embed --input-fasta in.fa --output-npz out.npz --model-name evo-1-8k-base --layers 16,final --pooling mean

The .npz holds `names` (the FASTA record names, in file order) and one array per layer, `layer_<k>` / `final`, in the same order:
[N, D] float32 for pooled modes, and for --pooling none the rows of every sequence concatenated ([sum of lengths, D]) with `offsets`
[N + 1] marking where each sequence's rows start."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def layer_key(layer) -> str:
    return "final" if layer == "final" else f"layer_{layer}"


def main():
    ap = argparse.ArgumentParser(description="Embed sequences with an Evo model on MI355X")
    ap.add_argument("--input-fasta", required=True)
    ap.add_argument("--output-npz", required=True)
    ap.add_argument("--model-name", default="evo-1-8k-base")
    ap.add_argument("--weights", default=None, help='checkpoint directory, or "synthetic"')
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--layers", default="final", help='comma-separated block indices and / or "final", e.g. 16,final')
    ap.add_argument("--pooling", default="mean", choices=["mean", "last", "none"])
    args = ap.parse_args()

    import numpy as np

    import evo_amd
    from evo_amd.embeddings import normalize_layers
    from evo_amd.fasta import length_buckets, read_fasta
    records = list(read_fasta(args.input_fasta))
    if not records:
        raise SystemExit(f"{args.input_fasta}: no FASTA records")
    names = [n for n, _ in records]
    seqs = [s for _, s in records]
    m = evo_amd.Evo(args.model_name, device=args.device, weights=args.weights)
    m.model.eval()
    layers = normalize_layers(args.layers, m.model.num_layers)
    got = {l: [None] * len(seqs) for l in layers}
    for idxs in length_buckets(seqs, args.batch_size):
        emb = evo_amd.embed_sequences([seqs[i] for i in idxs], m.model, m.tokenizer, layers=layers, pooling=args.pooling,
                                      device=args.device)
        for l in layers:
            for j, i in enumerate(idxs):
                got[l][i] = emb[l][j]
    arrays = {"names": np.array(names)}
    for l in layers:
        if args.pooling == "none":
            arrays[layer_key(l)] = np.concatenate(got[l], axis=0)
        else:
            arrays[layer_key(l)] = np.stack(got[l], axis=0)
    if args.pooling == "none":
        arrays["offsets"] = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.int64)
    np.savez(args.output_npz, **arrays)


if __name__ == "__main__":
    main()
