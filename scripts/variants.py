#!/usr/bin/env python
"""Reference + variants -> variant-effect scores (companion of scripts/score.py and scripts/profile.py: same model flags).

    python -m scripts.variants --reference ref.fa --variants vars.fa --output-tsv out.tsv
    python -m scripts.variants --reference ref.fa --scan --positions 100-199 --output-tsv scan.tsv

--reference holds ONE record.  --variants: a FASTA of full-length variant sequences (substitutions, multi-mutants, insertions,
deletions, truncations); --scan: every single substitution of the reference by A / C / G / T, optionally only at --positions a-b
(0-based, inclusive).  One line per variant: name, first_diff (index of the first changed token, BOS = 0; -1 = the reference itself),
score (as scripts/score.py gives it) and delta = log-likelihood(variant) - log-likelihood(reference), summed over all tokens."""
import argparse
import os
import sys

_HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:] = [p for p in sys.path if os.path.abspath(p or os.getcwd()) != _HERE]
sys.path.insert(0, os.path.dirname(_HERE))


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(description="Variant-effect scores from cached prefixes of one reference, with an Evo model on MI355X")
    ap.add_argument("--reference", required=True, help="FASTA with one record")
    src = ap.add_mutually_exclusive_group(required=True)
    src.add_argument("--variants", default=None, help="FASTA of full-length variants")
    src.add_argument("--scan", action="store_true", help="all single substitutions of the reference")
    ap.add_argument("--positions", default=None, help="with --scan: a-b, 0-based inclusive nucleotide positions")
    ap.add_argument("--output-tsv", required=True)
    ap.add_argument("--checkpoint-every", type=int, default=512)
    ap.add_argument("--reduce-method", default="mean", choices=["mean", "sum"])
    ap.add_argument("--model-name", default="evo-1-8k-base")
    ap.add_argument("--weights", default=None, help='checkpoint directory, or "synthetic"')
    ap.add_argument("--device", default="cuda:0")
    return ap


def parse_positions(text, length):
    if text is None:
        return None
    try:
        a, b = (int(x) for x in text.split("-"))
    except ValueError:
        raise ValueError(f"--positions: expected a-b, got {text!r}")
    if not 0 <= a <= b < length:
        raise ValueError(f"--positions {text}: outside the reference (length {length})")
    return range(a, b + 1)


def run(args, model, tokenizer):
    """-> (names, VariantScores)"""
    from evo_amd.fasta import read_fasta
    from evo_amd.scoring import score_variants, single_substitutions
    ref = [(n, s) for n, s in read_fasta(args.reference)]
    if len(ref) != 1 or not ref[0][1]:
        raise SystemExit(f"{args.reference}: expected exactly one non-empty record")
    ref_name, ref_seq = ref[0]
    if args.scan:
        subs = single_substitutions(ref_seq, parse_positions(args.positions, len(ref_seq)))
        names = [f"{ref_name}:{ref_seq[p]}{p}{alt}" for p, alt, _ in subs]
        seqs = [s for _, _, s in subs]
    else:
        recs = [(n, s) for n, s in read_fasta(args.variants)]
        if not recs or any(not s for _, s in recs):
            raise SystemExit(f"{args.variants}: no records, or a record without a sequence")
        names, seqs = [n for n, _ in recs], [s for _, s in recs]
    res = score_variants(ref_seq, seqs, model, tokenizer, reduce_method=args.reduce_method, checkpoint_every=args.checkpoint_every,
                         device=args.device)
    return names, res


def write_tsv(path, names, res) -> None:
    with open(path, "w") as f:
        f.write("name\tfirst_diff\tscore\tdelta\n")
        f.write(f"#reference\t-1\t{float(res.reference_score)!r}\t0.0\n")
        for n, d, s, dl in zip(names, res.first_diff, res.score, res.delta):
            f.write(f"{n}\t{int(d)}\t{float(s)!r}\t{float(dl)!r}\n")


def main(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.positions is not None and not args.scan:
        ap.error("--positions goes with --scan")
    if args.checkpoint_every <= 0 or args.checkpoint_every % 64:
        ap.error("--checkpoint-every must be a positive multiple of 64")
    import evo_amd
    m = evo_amd.Evo(args.model_name, device=args.device, weights=args.weights)
    m.model.eval()
    names, res = run(args, m.model, m.tokenizer)
    write_tsv(args.output_tsv, names, res)
    print(f"{len(names)} variants: {res.stats['tokens']} tokens forwarded in {res.stats['passes']} passes "
          f"(one forward per variant: {res.stats['naive_tokens']}), checkpoints {res.stats['checkpoints']}")


if __name__ == "__main__":
    main()
