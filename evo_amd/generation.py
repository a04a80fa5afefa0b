"""Sampling with the reference's `Generator.generate` / `generate` interface [REF evo/generation.py:13-297].

The token loop stays host-side Python, as in the reference.  Two deliberate differences:

1. Prompt handling.  The reference prefills only the first `force_prompt_threshold` (default 128)
   prompt tokens in parallel and pushes the rest through the recurrence one token at a time
   [REF evo/generation.py:81-88,131-189], because upstream's FFT prefill materialises [B,D,8,2T]
   temporaries.  This engine's long-convolution kernel already ends with the exact modal state, so
   by default (`force_prompt_threshold=None`) the WHOLE prompt is prefilled in one parallel pass.
   Passing an integer threshold reproduces the reference's schedule.
2. Cache offsets.  After its short prefill the reference jumps `seqlen_offset` to the full prompt
   length [REF evo/generation.py:142-145], so teacher-forced tokens get rotary positions starting at P
   and KV rows [threshold, P) are never written.  Here the offset always equals the
   number of tokens actually cached; `legacy_offsets=True` restores the reference behaviour.

The shifted score pairing of the wrapper [REF evo/generation.py:287; evo/scoring.py:48-50] is kept
verbatim so reported scores match.
"""
import sys
from typing import List, Tuple

import numpy as np
import torch

from .scoring import logits_to_logprobs, prepare_batch
from .sh.cache import W8_MAX_ROWS, check_kv_dtype, check_weight_dtype, check_weight_rows
from .sh.sample import allowed_mask, sample
from .tokenizer import CharLevelTokenizer


def w8_rows(model) -> int:
    """Batch rows the FP8-weight launches of this model's backend serve (Backend.W8_ROWS; 8 where a backend declares nothing)."""
    return int(getattr(getattr(model, "ops", None), "W8_ROWS", W8_MAX_ROWS))


def check_fp8_weight_model(model, rows: int = 1) -> None:
    """weight_dtype="fp8" on this model at `rows` batch rows: RuntimeError without the "w_fp8" kernels, ValueError for a streamed layer
    the launches cannot take (K % 16 != 0; above 8 rows K % 256 != 0) -- from shapes alone, before any device
    work."""
    ops = getattr(model, "ops", None)
    if ops is None or not hasattr(ops, "supports") or not ops.supports("w_fp8"):
        raise RuntimeError('weight_dtype="fp8" needs a compute backend with the "w_fp8" kernels (w_quant_fp8 and the *_w8 dense launches); '
                           "this model's backend has none")
    if rows > W8_MAX_ROWS:
        model.check_fp8_weights(rows)
    else:
        model.check_fp8_weights()


class Generator:
    def __init__(self, model, tokenizer: CharLevelTokenizer, top_k: int = 50, top_p: float = 0.7,
                 temperature: float = 1.0, seed: int = None, allowed_tokens=None, kv_dtype: str = "bf16",
                 weight_dtype: str = "bf16"):
        """`seed` / `allowed_tokens` (additions to the reference's interface, off by default): with either, tokens are drawn by
        the device sampler `evo_sample_rows_f32` -- row b of a batch draws from random stream `stream_offset + b`, reproducibly
        under `seed`, and only from `allowed_tokens` (e.g. "ACGT") when given.  `kv_dtype="fp8"`: the caches this
        generator creates hold their K/V in FP8 e4m3fn.  `weight_dtype="fp8"`: the single-token steps on those caches
        stream FP8 e4m3fn copies of the dense weights (batches of up to 64 prompts on the HIP backend; DESIGN.md sections 22 and 28: more memory,
        fewer bytes per token)."""
        self.kv_dtype = check_kv_dtype(kv_dtype)
        self.weight_dtype = check_weight_dtype(weight_dtype)
        if self.weight_dtype == "fp8":
            check_fp8_weight_model(model)
        if self.kv_dtype == "fp8" and not (hasattr(model, "ops") and model.ops.supports("kv_fp8")):
            raise RuntimeError('kv_dtype="fp8" needs a compute backend with the "kv_fp8" kernels (kv_quant_fp8, rope_append_decode_fp8, '
                               "attention_decode_fp8); this model's backend has none")
        self.model = model
        self.tokenizer = tokenizer
        self.top_k = top_k
        self.top_p = top_p
        self.temperature = temperature
        self.untils = ["\n\n"]
        self.device_sampler = seed is not None or allowed_tokens is not None
        self.seed = 0 if seed is None else int(seed)
        self.allow_mask = None if allowed_tokens is None else allowed_mask(tokenizer, allowed_tokens)
        self.stream_offset = 0                               # first random stream of the next batch (advanced by `generate`)

    def _rehome_cache(self, cache: dict, device) -> None:
        """Cached tensors follow the input's device [REF evo/generation.py:105-114]."""
        for store in (cache["mha"].key_value_memory_dict, cache["hyena"].fir_state_dict,
                      cache["hyena"].state_dict):
            for key, t in store.items():
                store[key] = t.to(device)                    # (an Fp8KV record moves both of its tensors)

    def generate(self, device: str, input_string: str = None, input_ids: torch.Tensor = None,
                 num_tokens: int = 32, cached_generation: bool = True, force_prompt_threshold: int = None,
                 print_generation: bool = True, verbose: bool = False, skip_special_tokens: bool = False,
                 stop_at_eos: bool = True, max_seqlen: int = None, inference_params_dict: dict = None,
                 legacy_offsets: bool = False) -> Tuple[torch.Tensor, torch.Tensor, dict]:
        """Returns (generated ids [B, n], the logits that produced them [B, n, V] f32, cache dict)."""
        tok = self.tokenizer
        eos_ids = torch.LongTensor([tok.eos]).to(device) if isinstance(tok.eos, int) \
            else tok.tokenize(tok.eos).to(device)
        if input_ids is None:
            enc = tok.tokenize(input_string)
            prompt = torch.LongTensor([int(t) for t in enc]).unsqueeze(0).to(device) if isinstance(enc, list) \
                else enc.unsqueeze(0).to(device)
        else:
            prompt = input_ids
        x = prompt if max_seqlen is None else prompt[:, -max_seqlen:]

        num_tokens = int(num_tokens)
        B, P = x.shape
        if self.weight_dtype == "fp8":
            check_weight_rows(B, "prompts in the batch", w8_rows(self.model))
            check_fp8_weight_model(self.model, B)
        x_force = None
        n_forced = 0
        if force_prompt_threshold is not None and P > force_prompt_threshold:
            n_forced = P - force_prompt_threshold
            x_force = x[:, force_prompt_threshold:]
            x = x[:, :force_prompt_threshold]

        generation = torch.empty(B, num_tokens, dtype=torch.long, device=x.device)
        scores = torch.empty(B, num_tokens, tok.vocab_size, dtype=torch.float, device=x.device)

        prefilled = False
        if inference_params_dict is not None:
            if any(getattr(c, "lengths", None) is not None for c in inference_params_dict.values()):
                raise ValueError("Generator cannot continue a ragged prefill (StripedHyena.prefill_ragged): its rows end at different positions "
                                 "and the scalar seqlen_offset of this loop describes one; decode such a cache per row (DecodePool)")
            cached_generation = True
            prefilled = True
            self._rehome_cache(inference_params_dict, x.device)
        elif cached_generation:
            inference_params_dict = self.model.initialize_inference_params()
            inference_params_dict["mha"].max_batch_size = B
            inference_params_dict["hyena"].max_batch_size = B
            inference_params_dict["mha"].kv_dtype = self.kv_dtype
        if inference_params_dict is not None:                # (a cache handed in continues in this generator's weight format)
            inference_params_dict["mha"].weight_dtype = self.weight_dtype

        if verbose:
            print("Starting generation...")
            print("Prompt: " + input_string if input_string is not None else f"Prompt ids: {input_ids} {input_ids.shape}")

        if self.device_sampler:                              # per-row settings and stream ids of the device sampler, made once
            ops = self.model.ops
            s_top_k = torch.full((B,), int(self.top_k), dtype=torch.int32, device=x.device)
            s_top_p = torch.full((B,), float(self.top_p), dtype=torch.float32, device=x.device)
            s_temp = torch.full((B,), float(self.temperature), dtype=torch.float32, device=x.device)
            s_stream = torch.arange(B, dtype=torch.int64, device=x.device) + self.stream_offset
            s_count = torch.zeros(B, dtype=torch.int64, device=x.device)     # the kernel advances it: draw j has count j
            s_allow = None if self.allow_mask is None else ops.pack_allow_mask(self.allow_mask, x.device)
            self.stream_offset += B

        total_steps = n_forced + num_tokens
        i = -1
        for i in range(total_steps):
            post_prefill = prefilled or (cached_generation and i > 0)
            if post_prefill:
                x = x[:, -1:]
                mha, hy = inference_params_dict["mha"], inference_params_dict["hyena"]
                if mha.seqlen_offset == 0:
                    first = prompt.shape[-1] if legacy_offsets else (P - n_forced)
                    mha.seqlen_offset = hy.seqlen_offset = first
                else:
                    mha.seqlen_offset += 1
                    hy.seqlen_offset += 1
            with torch.inference_mode():
                logits, inference_params_dict = self.model(x, inference_params_dict=inference_params_dict)
            last_logits = logits[:, -1]

            if i < n_forced:
                new_idx = x_force[:, i]                               # teacher forcing of the prompt tail
            else:
                if self.device_sampler:
                    new_idx = ops.sample_rows(last_logits, s_top_k, s_top_p, s_temp, self.seed, stream=s_stream, count=s_count,
                                              allow=s_allow)[0]
                else:
                    new_idx = sample(last_logits, top_k=self.top_k, top_p=self.top_p, temperature=self.temperature)
                j = i - n_forced
                scores[:, j] = last_logits
                generation[:, j] = new_idx

            if stop_at_eos and num_tokens >= 2 and bool((generation[0, -2:] == eos_ids).all()):
                print("Stopping generation at EOS")
            if print_generation and verbose and B == 1:
                print(f"{tok.detokenize([new_idx.item()])}", end=" ")

            x = new_idx[:, None] if post_prefill else torch.cat([x, new_idx[:, None]], dim=-1)

        if verbose:
            y = tok.detokenize_batch(generation[:, : i + 1])
            for until in self.untils:
                if until in y:
                    y = y.split(until)[0]
                    break
            print(f"\nInput: {input_string}, Output: {y}")
        if hasattr(self.model, "release_decode_graph"):
            self.model.release_decode_graph()                # the captured step pins the caches it was captured on
        return generation[:, : i + 1], scores[:, : i + 1], inference_params_dict


def generate(prompt_seqs: List[str], model, tokenizer: CharLevelTokenizer, n_tokens: int = 100,
             temperature: float = 0.0, top_k: int = 1, top_p: float = 1.0, batched: bool = True,
             prepend_bos: bool = False, cached_generation: bool = False, force_prompt_threshold: int = None,
             verbose: int = 1, device: str = "cuda:0", seed: int = None, allowed_tokens=None, kv_dtype: str = "bf16",
             weight_dtype: str = "bf16", **kwargs) -> Tuple[List[str], List[float]]:
    """Generate `n_tokens` after each prompt.  Equal-length prompts run as one batch when `batched`.
    Returns (generated strings, mean log-likelihood score per generation).  `seed`: the same call gives the same strings
    (prompt number i draws from random stream i); `allowed_tokens`: the characters that may be generated, e.g. "ACGT"; `kv_dtype="fp8"`
    (with `cached_generation`): the KV cache in FP8 e4m3fn; `weight_dtype="fp8"` (with `cached_generation`, batches of up to 64 prompts): the
    decode steps stream FP8 copies of the dense weights (DESIGN.md sections 22 and 28)."""
    if hasattr(model, "eval"):
        model.eval()
    g = Generator(model, tokenizer, top_k=top_k, top_p=top_p, temperature=temperature, seed=seed, allowed_tokens=allowed_tokens,
                  kv_dtype=kv_dtype, weight_dtype=weight_dtype)

    same_len = all(len(s) == len(prompt_seqs[0]) for s in prompt_seqs)
    if batched and same_len:
        if weight_dtype == "fp8":
            check_weight_rows(len(prompt_seqs), "prompts in the batch", w8_rows(model))
            check_fp8_weight_model(model, len(prompt_seqs))
        batches = [prepare_batch(prompt_seqs, tokenizer, prepend_bos=prepend_bos, device=device)[0]]
    else:
        if verbose:
            if not same_len:
                sys.stderr.write("Note: Prompts are of different lengths.\n")
            sys.stderr.write("Note: Will not do batched generation.\n")
        batches = [prepare_batch([s], tokenizer, prepend_bos=prepend_bos, device=device)[0] for s in prompt_seqs]

    seqs_out: List[str] = []
    scores_out: List[float] = []
    for input_ids in batches:
        bsz = input_ids.shape[0]
        output_ids, logits, _ = g.generate(
            input_ids=input_ids, num_tokens=n_tokens, cached_generation=cached_generation,
            force_prompt_threshold=force_prompt_threshold, device=device, print_generation=(verbose > 1),
            verbose=(verbose > 1), stop_at_eos=False, legacy_offsets=bool(kwargs.get("legacy_offsets", False)))
        if verbose > 1:
            print("input_ids.shape", input_ids.shape)
            print("output_ids.shape", output_ids.shape)
            print("logits.shape", logits.shape)
        decoded = list(tokenizer.detokenize_batch(output_ids))
        assert len(decoded) == bsz
        seqs_out += decoded
        # same pairing as the reference: logits j vs token j+1 (default trim_bos=True)
        lp = logits_to_logprobs(logits, output_ids).float().cpu().numpy()
        scores_out += [np.mean(lp[b]) for b in range(bsz)]

    assert len(seqs_out) == len(scores_out) == len(prompt_seqs)
    if verbose:
        for seq, score, prompt in zip(seqs_out, scores_out, prompt_seqs):
            print(f'Prompt: "{prompt}",\tOutput: "{seq}",\tScore: {score}')
    return seqs_out, scores_out
