#!/usr/bin/env python
"""FASTA -> per-position nucleotide profiles (companion of scripts/score.py and scripts/embed.py: same model flags, sequences bucketed
by length before batching).

    python -m scripts.profile --input-fasta in.fa --output-npz out.npz --output-tsv out.tsv --tokens ACGT --model-name evo-1-8k-base

For every record and every position i: the log-prob of the observed base seq[i] given seq[:i], the entropy of the model's
distribution there, and the log-prob of each token of --tokens -- one forward per batch, the fused tail's profile epilogue.
  .npz  `names` (record names, file order), `tokens` (the token ids, column order) and per record `<name>/logprob` [L],
        `<name>/entropy` [L], `<name>/token_logprobs` [L, n], all float32
  .tsv  long form, one line per position: name, pos (0-based), ref, logprob, entropy, then one column per token"""
import argparse
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
# run as a file, this directory leads sys.path and `import profile` (the standard library's profiler, which cProfile imports) would find
# THIS file: take the directory out before anything else is imported
sys.path[:] = [p for p in sys.path if os.path.abspath(p or os.getcwd()) != _HERE]
sys.path.insert(0, os.path.dirname(_HERE))


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Per-position token profiles (log-probs of A, C, G, T ...) with an Evo model on MI355X")
    ap.add_argument("--input-fasta", required=True)
    ap.add_argument("--output-npz", default=None)
    ap.add_argument("--output-tsv", default=None)
    ap.add_argument("--tokens", default="ACGT", help="1 to 8 distinct ASCII characters: the columns of the profile")
    ap.add_argument("--batch-size", type=int, default=8)
    ap.add_argument("--model-name", default="evo-1-8k-base")
    ap.add_argument("--weights", default=None, help='checkpoint directory, or "synthetic"')
    ap.add_argument("--device", default="cuda:0")
    return ap


def token_label(t: int) -> str:
    """Column header of token id t: the character itself when it is printable ASCII, `id<t>` otherwise."""
    return chr(t) if 33 <= t < 127 else f"id{t}"


def write_npz(path, names, profiles) -> None:
    import numpy as np
    if len(set(names)) != len(names):
        raise ValueError("record names repeat: the .npz keys are <name>/logprob ...")
    arrays = {"names": np.array(names), "tokens": np.asarray(profiles[0].tokens if profiles else (), dtype=np.int64)}
    for n, p in zip(names, profiles):
        arrays[f"{n}/logprob"] = p.logprob.astype(np.float32)
        arrays[f"{n}/entropy"] = p.entropy.astype(np.float32)
        arrays[f"{n}/token_logprobs"] = p.token_logprobs.astype(np.float32)
    np.savez(path, **arrays)


def write_tsv(path, names, seqs, profiles) -> None:
    with open(path, "w") as f:
        tokens = profiles[0].tokens if profiles else ()
        f.write("\t".join(["name", "pos", "ref", "logprob", "entropy"] + [token_label(t) for t in tokens]) + "\n")
        for n, s, p in zip(names, seqs, profiles):
            for i, ch in enumerate(s):
                cols = [n, str(i), ch, repr(float(p.logprob[i])), repr(float(p.entropy[i]))]
                f.write("\t".join(cols + [repr(float(v)) for v in p.token_logprobs[i]]) + "\n")


def run(args, model, tokenizer):
    """The profiles of every FASTA record, in file order -> (names, seqs, profiles)."""
    from evo_amd.fasta import length_buckets, read_fasta
    from evo_amd.scoring import position_profiles, profile_token_ids
    tokens = profile_token_ids(args.tokens)
    records = [(n, s) for n, s in read_fasta(args.input_fasta)]
    if not records:
        raise SystemExit(f"{args.input_fasta}: no FASTA records")
    if any(not s for _, s in records):
        raise SystemExit(f"{args.input_fasta}: a record has no sequence")
    names = [n for n, _ in records]
    seqs = [s for _, s in records]
    profiles = [None] * len(seqs)
    for idxs in length_buckets(seqs, args.batch_size):
        got = position_profiles([seqs[i] for i in idxs], model, tokenizer, tokens=tokens, device=args.device)
        for i, p in zip(idxs, got):
            profiles[i] = p
    return names, seqs, profiles


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if not args.output_npz and not args.output_tsv:
        ap.error("give --output-npz and / or --output-tsv")
    from evo_amd.scoring import profile_token_ids
    try:
        profile_token_ids(args.tokens)
    except ValueError as e:
        ap.error(str(e))

    import evo_amd
    m = evo_amd.Evo(args.model_name, device=args.device, weights=args.weights)
    m.model.eval()
    names, seqs, profiles = run(args, m.model, m.tokenizer)
    if args.output_npz:
        write_npz(args.output_npz, names, profiles)
    if args.output_tsv:
        write_tsv(args.output_tsv, names, seqs, profiles)


if __name__ == "__main__":
    main()
