#!/usr/bin/env python
"""Beam search: the `--beam-width` most likely continuations of every prompt, by total log-probability.  Prompts
(any lengths) from a FASTA / text file; CSV out, one row per hypothesis: Prompt Id, Rank, Sequence, Score, Length.

    python -m scripts.beam_search --prompts p.fa --output-csv out.csv --beam-width 4 --n-tokens 256 --allowed-tokens ACGT --stop-tokens N
"""
import argparse
import csv
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from scripts.sample_many import read_prompts  # noqa: E402


def main(argv=None):
    ap = argparse.ArgumentParser(description="Beam search with an Evo model on MI355X")
    ap.add_argument("--prompts", required=True, help="FASTA or one-prompt-per-line text file")
    ap.add_argument("--output-csv", required=True)
    ap.add_argument("--model-name", default="evo-1-8k-base")
    ap.add_argument("--beam-width", type=int, default=4, help="hypotheses kept per prompt (1 ... 8)")
    ap.add_argument("--n-tokens", type=int, default=256, help="tokens a hypothesis may grow to")
    ap.add_argument("--n-slots", type=int, default=None, help="decode streams advanced together per step (default: beam width x "
                                                              "min(prompts, 32 // beam width))")
    ap.add_argument("--allowed-tokens", default=None, help='characters that may be generated, e.g. "ACGT" (default: any byte)')
    ap.add_argument("--stop-tokens", default=None, help='characters that end a hypothesis and are trimmed from it, e.g. "N"')
    ap.add_argument("--prefill-batch", type=int, default=1, help="prefill up to N prompts admitted together in one forward")
    ap.add_argument("--weight-dtype", choices=["bf16", "fp8"], default="bf16", help="dense weights the decode step streams (fp8: up to 64 slots)")
    ap.add_argument("--prepend-bos", action="store_true")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--weights", default=None)
    args = ap.parse_args(argv)
    if not 1 <= args.beam_width <= 8:
        ap.error("--beam-width must be 1 ... 8")
    if args.n_tokens < 1:
        ap.error("--n-tokens must be >= 1")
    if args.n_slots is not None and args.n_slots < args.beam_width:
        ap.error("--n-slots must hold at least one beam group")

    import evo_amd
    prompts = read_prompts(args.prompts)
    if not prompts:
        raise SystemExit(f"no prompts in {args.prompts}")
    m = evo_amd.Evo(args.model_name, device=args.device, weights=args.weights)
    results = evo_amd.beam_search(prompts, m.model, m.tokenizer, n_tokens=args.n_tokens, beam_width=args.beam_width, n_slots=args.n_slots,
                                  allowed_tokens=args.allowed_tokens, stop_tokens=args.stop_tokens or None, prefill_batch=args.prefill_batch,
                                  weight_dtype=args.weight_dtype, device=args.device, prepend_bos=args.prepend_bos)
    rows = [[str(pi), str(rank), seq, repr(score), str(length)]
            for pi, r in enumerate(results) for rank, (seq, score, length) in enumerate(zip(r.sequences, r.scores, r.lengths))]
    with open(args.output_csv, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["Prompt Id", "Rank", "Sequence", "Score", "Length"])
        w.writerows(rows)
    print(f"{len(rows)} hypotheses of at most {args.n_tokens} tokens for {len(prompts)} prompts (beam width {args.beam_width}) -> {args.output_csv}")
    return rows


if __name__ == "__main__":
    main()
