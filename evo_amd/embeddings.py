"""Sequence embeddings: the hidden representation of every DNA sequence at chosen blocks and / or the final norm, mean-pooled
(or last-token, or per position) -- what evo users build downstream classifiers and regressors on.

    emb = evo_amd.embed_sequences(seqs, m.model, m.tokenizer, layers=(16, "final"))     # {16: [N, D], "final": [N, D]} float32

The forward runs once, up to the deepest requested block (StripedHyena.embeddings: early exit, no unembedding), and every
requested stream is pooled on the device by the pooling kernel (csrc/pool.hip) as soon as its block finishes."""
from typing import Dict, List, Sequence, Union

import numpy as np
import torch

from .scoring import prepare_batch
from .tokenizer import CharLevelTokenizer

POOLINGS = ("mean", "last", "none")


def normalize_layers(layers, num_layers: int) -> List[Union[int, str]]:
    """Checks a `layers` argument: a non-empty list of block indices in [0, num_layers) and / or "final" (no duplicates).  A string
    like "16,final" is accepted too (the CLI's form)."""
    if isinstance(layers, str):
        layers = [s.strip() for s in layers.split(",") if s.strip()]
    elif isinstance(layers, (int, np.integer)):
        layers = [layers]
    out: List[Union[int, str]] = []
    for l in layers:
        if isinstance(l, str) and l != "final":
            if not l.lstrip("-").isdigit():
                raise ValueError(f"layer {l!r}: expected a block index or 'final'")
            l = int(l)
        if not isinstance(l, str):
            if isinstance(l, bool) or not isinstance(l, (int, np.integer)):
                raise ValueError(f"layer {l!r}: expected a block index or 'final'")
            l = int(l)
            if not 0 <= l < num_layers:
                raise ValueError(f"layer {l} is outside [0, {num_layers})")
        if l in out:
            raise ValueError(f"layer {l!r} is requested twice")
        out.append(l)
    if not out:
        raise ValueError("layers is empty")
    return out


def check_pooling(pooling: str) -> str:
    if pooling not in POOLINGS:
        raise ValueError(f"pooling must be one of {POOLINGS}, got {pooling!r}")
    return pooling


def embed_sequences(seqs: Sequence[str], model, tokenizer: CharLevelTokenizer, layers=("final",), pooling: str = "mean",
                    device: str = "cuda:0") -> Dict[Union[int, str], Union[np.ndarray, List[np.ndarray]]]:
    """Embeddings of `seqs` (one batch: callers with many sequences bucket them by length, as scripts/embed.py does).

    layers:  block indices k (the residual stream leaving block k) and / or "final" (the final-norm output).
    pooling: "mean" over the sequence's own positions (BOS and pads excluded), "last" (its last nucleotide), or "none".
    Returns {layer: np.ndarray [N, D] float32} for pooled modes, {layer: [np.ndarray [len_i, D] float32, ...]} for "none"."""
    seqs = list(seqs)
    if not seqs:
        raise ValueError("embed_sequences: no sequences given")
    if any(len(s) == 0 for s in seqs):
        raise ValueError("embed_sequences: empty sequence")
    layers = normalize_layers(layers, int(model.num_layers))
    check_pooling(pooling)
    input_ids, lengths = prepare_batch(seqs, tokenizer, prepend_bos=True, device=device)
    with torch.inference_mode():
        got = model.embeddings(input_ids, layers, pooling=pooling, start=1, lengths=lengths)
    if pooling != "none":
        return {l: got[l].float().cpu().numpy() for l in layers}
    out = {}
    for l in layers:
        rows = got[l].float().cpu().numpy()                 # [N, T, D]
        out[l] = [rows[i, 1:1 + n] for i, n in enumerate(lengths)]
    return out
