#!/usr/bin/env python
"""Many prompts x many samples with continuous batching -- the `semantic_design.sample_model` job
[REF semantic_design/semantic_design.py:271-400]: prompts (any lengths) from a FASTA / text file, `--n-sample-per-prompt`
generations of `--n-tokens` each, CSV out with the reference's columns (UUID, Prompt, Generated Sequence, Score).

    python -m scripts.sample_many --prompts prompts.fasta --output-csv out.csv --n-sample-per-prompt 8 --n-slots 16

Jobs that end on their own: `--n-tokens` becomes a limit, a generation ends at its first in-frame stop codon

    python -m scripts.sample_many --prompts prompts.fasta --output-csv out.csv --allowed-tokens ACGT \
        --stop-sequences TAA,TAG,TGA --stop-frame 3 --scores-only --extra-columns

Constrained generation: every generation fills an IUPAC template, encodes a protein, or is an open reading frame

    python -m scripts.sample_many --prompts prompts.fasta --output-csv out.csv --allowed-tokens ACGT --template ATGNNNNNNRRYNNNTAA
    python -m scripts.sample_many --prompts prompts.fasta --output-csv out.csv --allowed-tokens ACGT --encode-protein MKLS*
    python -m scripts.sample_many --prompts prompts.fasta --output-csv out.csv --allowed-tokens ACGT --orf-min-codons 50

k-mer repeat control: nucleotides that would complete an 8-mer the generation (or its prompt) already holds are
penalised, and a generation of which more than 30 % is such repeats ends early

    python -m scripts.sample_many --prompts prompts.fasta --output-csv out.csv --allowed-tokens ACGT --repeat-k 8 \
        --repeat-end-fraction 0.3 --extra-columns
"""
import argparse
import csv
import math
import os
import sys
import uuid

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def read_prompts(path: str):
    """FASTA (records) or plain text (one prompt per non-empty line)."""
    from evo_amd.fasta import read_fasta
    with open(path) as f:
        head = f.read(1)
    if head == ">":
        return [seq for _, seq in read_fasta(path) if seq.strip()]
    with open(path) as f:
        return [ln.strip() for ln in f if ln.strip()]


def main(argv=None):
    ap = argparse.ArgumentParser(description="Sample many sequences from an Evo model on MI355X (continuous batching)")
    ap.add_argument("--prompts", required=True, help="FASTA or one-prompt-per-line text file")
    ap.add_argument("--output-csv", required=True)
    ap.add_argument("--model-name", default="evo-1-8k-base")
    ap.add_argument("--n-tokens", type=int, default=1000)
    ap.add_argument("--n-sample-per-prompt", type=int, default=1)
    ap.add_argument("--temperature", type=float, default=0.7)
    ap.add_argument("--top-k", type=int, default=4)
    ap.add_argument("--top-p", type=float, default=1.0)
    ap.add_argument("--n-slots", type=int, default=16, help="decode streams advanced together per step")
    ap.add_argument("--prepend-bos", action="store_true")
    ap.add_argument("--seed", type=int, default=None, help="reproducible run (for a fixed --n-slots): every sample draws from its own "
                                                           "random stream; the sampler then runs on the device")
    ap.add_argument("--allowed-tokens", default=None, help='characters that may be generated, e.g. "ACGT" (default: any byte)')
    ap.add_argument("--share-prompt-kv", action="store_true", help="the samples of a prompt read ONE stored copy of its K/V instead of a "
                                                                   "private copy per decode stream (long prompts, many samples)")
    ap.add_argument("--prefill-batch", type=int, default=1, help="prefill up to N prompts admitted together in one forward, right-padded "
                                                                 "(default 1: every prompt alone)")
    ap.add_argument("--stop-tokens", default=None, help='characters that end a generation and are trimmed from it, e.g. "N"')
    ap.add_argument("--stop-sequences", default=None, help="comma-separated patterns of 1-8 characters (at most 8) that end a generation and "
                                                           "stay in it, e.g. TAA,TAG,TGA")
    ap.add_argument("--stop-frame", type=int, default=1, help="a stop sequence counts only when it ends at a multiple of this many generated "
                                                              "tokens (3: in-frame codons)")
    ap.add_argument("--scores-only", action="store_true", help="keep no logits, on the device or on the host: the scores come from the "
                                                               "sampler's own log-probabilities")
    ap.add_argument("--extra-columns", action="store_true", help="append Length and Finish (stop_token | stop_sequence | constraint | length | "
                                                                 "repeat) to the CSV, and Repeats with --repeat-k")
    ap.add_argument("--template", default=None, metavar="IUPAC", help="every generation fills this template of IUPAC nucleotide codes, "
                                                                      "e.g. ATGNNNNNNRRYNNNTAA")
    ap.add_argument("--encode-protein", default=None, metavar="SEQ", help="every generation is DNA that encodes this protein (one-letter "
                                                                          "residues, * = a stop codon): the model chooses the codons")
    ap.add_argument("--orf-min-codons", type=int, default=None, metavar="N", help="every generation is an open reading frame: ATG, no in-frame "
                                                                                  "stop codon before codon N, then the first one ends it")
    ap.add_argument("--then", choices=["end", "free"], default="end", help="what follows a completed --template / --encode-protein: the "
                                                                           "generation ends (default) or goes on unconstrained")
    ap.add_argument("--kv-dtype", choices=["bf16", "fp8"], default="bf16", help="format of the pool's KV cache; fp8 (e4m3fn with one scale per "
                                                                                "cached row) holds about half the bytes; not with "
                                                                                "--share-prompt-kv")
    ap.add_argument("--weight-dtype", choices=["bf16", "fp8"], default="bf16", help="dense weights the pool's decode step streams; fp8 (e4m3fn, "
                                                                                    "one scale per output row) halves the bytes per step and "
                                                                                    "adds an FP8 copy to memory; --n-slots up to 64")
    ap.add_argument("--kv-paged", action="store_true", help="keep the pool's KV cache in pages: a job holds what its own prompt and "
                                                            "limit need, not the longest job's; not with --share-prompt-kv or "
                                                            "--kv-dtype fp8")
    ap.add_argument("--kv-page-tokens", type=int, default=256, metavar="N", help="tokens per page with --kv-paged (a power of two >= 64)")
    ap.add_argument("--kv-budget-tokens", type=int, default=None, metavar="N", help="with --kv-paged: cap the page pool at N tokens; jobs "
                                                                                    "then wait for free pages, in order")
    ap.add_argument("--batch-invariant", action="store_true", help="with --seed: every generation is the same bits at any --n-slots from 1 to 64 "
                                                                   "(one launch sequence at every slot count; not with --prefill-batch > 1, "
                                                                   "--share-prompt-kv, --kv-dtype fp8 or --weight-dtype fp8)")
    ap.add_argument("--repeat-k", type=int, default=None, metavar="N", help="turn k-mer repeat control on: a nucleotide that would complete an "
                                                                            "N-mer the generation or its prompt already holds is penalised")
    ap.add_argument("--repeat-penalty", type=float, default=None, help="what is subtracted from such a nucleotide's logit per earlier "
                                                                       "occurrence of the N-mer (default 1.0)")
    ap.add_argument("--repeat-max-count", type=int, default=None, metavar="C", help="occurrences beyond C add nothing (default 4, at most 7)")
    ap.add_argument("--repeat-ignore-prompt", action="store_true", help="count the k-mers of the generation only, not those of its prompt")
    ap.add_argument("--repeat-end-fraction", type=float, default=None, metavar="F", help="end a generation (Finish: repeat) once more than "
                                                                                         "this fraction of it completed an N-mer seen before")
    ap.add_argument("--repeat-end-min-tokens", type=int, default=None, metavar="N", help="... but not before N tokens (default 64)")
    ap.add_argument("--device", default="cuda:0")
    ap.add_argument("--weights", default=None)
    args = ap.parse_args(argv)
    if args.kv_paged and (args.share_prompt_kv or args.kv_dtype != "bf16"):
        ap.error("--kv-paged does not combine with --share-prompt-kv or --kv-dtype fp8")
    if not args.kv_paged and (args.kv_page_tokens != 256 or args.kv_budget_tokens is not None):
        ap.error("--kv-page-tokens and --kv-budget-tokens apply with --kv-paged only")
    if args.kv_page_tokens < 64 or args.kv_page_tokens & (args.kv_page_tokens - 1):
        ap.error("--kv-page-tokens must be a power of two >= 64")
    if args.weight_dtype != "bf16" and args.n_slots > 64:
        ap.error("--weight-dtype fp8 serves pools of up to 64 slots")
    if args.batch_invariant and (args.n_slots > 64 or args.prefill_batch > 1 or args.share_prompt_kv or args.kv_dtype != "bf16"
                                 or args.weight_dtype != "bf16"):
        ap.error("--batch-invariant serves pools of up to 64 slots and does not combine with --prefill-batch > 1, --share-prompt-kv, "
                 "--kv-dtype fp8 or --weight-dtype fp8")
    if args.kv_dtype != "bf16" and args.share_prompt_kv:
        ap.error("--kv-dtype fp8 does not combine with --share-prompt-kv (the prompt store is bf16)")
    if args.repeat_k is None and (args.repeat_penalty is not None or args.repeat_max_count is not None or args.repeat_ignore_prompt
                                  or args.repeat_end_fraction is not None or args.repeat_end_min_tokens is not None):
        ap.error("--repeat-penalty, --repeat-max-count, --repeat-ignore-prompt, --repeat-end-fraction and --repeat-end-min-tokens apply "
                 "with --repeat-k only")
    if sum(x is not None for x in (args.template, args.encode_protein, args.orf_min_codons)) > 1:
        ap.error("at most one of --template, --encode-protein and --orf-min-codons")
    if args.then != "end" and args.template is None and args.encode_protein is None:
        ap.error("--then applies to --template and --encode-protein only (an open reading frame ends at its stop codon)")

    import evo_amd
    from evo_amd.pool import DecodePool
    prompts = read_prompts(args.prompts)
    if not prompts:
        raise SystemExit(f"no prompts in {args.prompts}")
    m = evo_amd.Evo(args.model_name, device=args.device, weights=args.weights)
    pool = DecodePool(m.model, m.tokenizer, n_slots=args.n_slots, top_k=args.top_k, top_p=args.top_p,
                      temperature=args.temperature, device=args.device, seed=args.seed, allowed_tokens=args.allowed_tokens,
                      share_prompt_kv=args.share_prompt_kv, prefill_batch=args.prefill_batch,
                      **({} if args.kv_dtype == "bf16" else {"kv_dtype": args.kv_dtype}),
                      **({"kv_paged": True, "kv_page_tokens": args.kv_page_tokens, "kv_budget_tokens": args.kv_budget_tokens}
                         if args.kv_paged else {}),
                      **({} if args.weight_dtype == "bf16" else {"weight_dtype": args.weight_dtype}),
                      **({"batch_invariant": True} if args.batch_invariant else {}))
    ctl = {}                                                  # any of these moves the job onto the job-control path
    if args.stop_tokens:
        ctl["stop_tokens"] = args.stop_tokens
    if args.stop_sequences:
        ctl["stop_sequences"] = [p for p in args.stop_sequences.split(",") if p]
    if args.stop_frame != 1:
        ctl["stop_frame"] = args.stop_frame
    if args.scores_only:
        ctl["return_logits"] = False
    if args.template is not None:
        ctl["constraints"] = evo_amd.iupac_template(args.template, then=args.then)
    elif args.encode_protein is not None:
        ctl["constraints"] = evo_amd.encode_protein(args.encode_protein, then=args.then)
    elif args.orf_min_codons is not None:
        ctl["constraints"] = evo_amd.open_reading_frame(args.orf_min_codons)
    if args.repeat_k is not None:
        ctl["repeat"] = evo_amd.RepeatControl(
            k=args.repeat_k, penalty=1.0 if args.repeat_penalty is None else args.repeat_penalty,
            max_count=4 if args.repeat_max_count is None else args.repeat_max_count, count_prompt=not args.repeat_ignore_prompt,
            end_fraction=args.repeat_end_fraction, end_min_tokens=64 if args.repeat_end_min_tokens is None else args.repeat_end_min_tokens)
    seqs, scores, owner = pool.generate(prompts, n_tokens=args.n_tokens, n_sample_per_prompt=args.n_sample_per_prompt,
                                        prepend_bos=args.prepend_bos, **ctl)
    extra = [[]] * len(seqs)
    if args.extra_columns:                                    # (without any of the options above every job runs to --n-tokens)
        extra = [[str(n), f] for n, f in zip(pool.last_lengths, pool.last_finish)] if ctl else [[str(args.n_tokens), "length"]] * len(seqs)
        if args.repeat_k is not None:                         # Repeats: generated tokens that completed a k-mer seen before
            extra = [x + [str(rep)] for x, (_, rep) in zip(extra, pool.last_repeats)]
    rows = [[uuid.uuid4().hex, prompts[o], s, str(sc)] + x for s, sc, o, x in zip(seqs, scores, owner, extra)
            if s.strip() and not math.isnan(sc)]              # the reference drops empty / NaN-scored generations
    with open(args.output_csv, "w", newline="") as f:
        w = csv.writer(f)
        w.writerow(["UUID", "Prompt", "Generated Sequence", "Score"] + (["Length", "Finish"] if args.extra_columns else [])
                   + (["Repeats"] if args.extra_columns and args.repeat_k is not None else []))
        w.writerows(rows)
    print(f"{len(rows)} generations of {'at most ' if ctl else ''}{args.n_tokens} tokens from {len(prompts)} prompts -> {args.output_csv} "
          f"({pool.stats['steps']} pooled steps, {pool.stats['prefills']} prefills)")
    return rows


if __name__ == "__main__":
    main()
