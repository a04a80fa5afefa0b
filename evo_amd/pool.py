"""Continuous batching of decode streams: the `semantic_design.sample_model` usage profile --
many prompts x `n_sample_per_prompt` generations of `n_tokens` each [REF semantic_design/semantic_design.py:271-360,
121-179].

The reference's `generate` batches only prompts of EQUAL length and otherwise generates one prompt at a time
[REF evo/generation.py:237-262]: a decode step streams all 12.9 GB of weights for a single token.  Here a fixed set
of `n_slots` decode streams shares every step.  Each slot owns one row of every cache tensor (KV rows, FIR history,
modal state) and its own position, held in DEVICE memory: the rotary table, the KV append and the split-K decode
attention all read per-row positions (`evo_attn_decode_bf16` dyn_pos[B]), so streams of different prompt lengths
and different ages advance together, a finished stream's slot is re-filled while the others keep going, and the
step has one shape for the whole job -- it is captured once in a hipGraph and replayed.

Prompts are prefilled one at a time (by default; `prefill_batch` > 1 below) with the ordinary parallel forward (the long-convolution kernel ends with the
exact modal state); the `n_sample_per_prompt` copies of a prompt share ONE prefill, whose caches are replicated
into their slots.  Sampling and scoring follow the reference wrapper verbatim (same `sample`, same shifted
logits/token pairing [REF evo/generation.py:162-167,287]), so with greedy sampling a pool run reproduces per-prompt
`generate` token for token (tests/test_pool.py).

With `seed` and / or `allowed_tokens` the sampler is the device kernel `evo_sample_rows_f32`: it is the
last node of the step (captured with it), writes the next ids where the next step reads them and appends tokens and logits to
a device-resident history, so the host reads nothing back per step -- a job's rows are copied out once, when its slot finishes.
Every job draws from its own random stream (its output index), so a sample does not depend on the slot it ran in, on the step
it was admitted at, or on the other prompts of the job -- for a fixed `n_slots` (the logits themselves depend on the row count).

`share_prompt_kv=True` (opt-in): the copies of a prompt no longer get a private copy of its K/V each.  A prompt's
K/V is installed ONCE into a row of a `PromptStore`; a slot's own cache holds only the `n_tokens` it generates, and the decode
attention reads the store row and then the slot's own keys (`HipOps.attention_decode_prefix`).  Which store row a slot continues, how
many keys that row holds and the slot's own index are device vectors, so the captured step still replays while slots are re-filled.

`prefill_batch=N` > 1 (opt-in): when a prompt needs a prefill, the distinct prompts among the jobs the idle slots are
about to take -- at most N, and at most `prefill_max_tokens` padded positions -- are prefilled in ONE forward of the right-padded batch
(`StripedHyena.prefill_ragged`); each slot is installed from its prompt's row of that batch.  With the default 1 nothing changes by a bit.

Jobs that end on their own (opt-in): with `stop_tokens`, `stop_sequences` / `stop_frame`, one `n_tokens` per prompt or
`return_logits=False`, `generate` runs on the sampler launch `evo_sample_rows_ctl_f32`: the row itself ends its job (stop token, in-frame
stop pattern, own limit) and goes inactive on the device.  The host knows the step by which a slot must have ended (its limit) and, with a
stop rule, reads one [S] vector of lengths every `poll_every` steps to learn who ended sooner; it fetches rows [:length] of the finished
slots' histories (tokens, log-probabilities, logits only when asked for), releases their store rows and re-fills them.

Constrained generation (opt-in): `generate(constraints=...)` gives every prompt (or some of them) a `TokenConstraint`
(evo_amd/constraints.py: an IUPAC template, a protein to encode, an open reading frame, concatenations).  The job-control path then ends
with the launch `evo_sample_rows_dfa_f32`: a slot's state in its prompt's automaton decides what it may draw, the token moves the state,
and completing the constraint ends the job -- all of it inside the captured step.

`kv_dtype="fp8"` (opt-in): the pool's KV cache holds FP8 e4m3fn rows with one power-of-two scale each (`Fp8KV`: 8,448
bytes per key and layer at 32 heads instead of 16,384; `stats["kv_bytes"]` reports what is held).  Prefills attend to their own bf16 keys
and only store quantised; the step appends with `rope_append_decode_fp8` and attends with `attention_decode_fp8`.  A pool has one format
for its life, so its captured step is captured on it.  Not with `share_prompt_kv` (ValueError): the prompt store stays bf16.

`weight_dtype="fp8"` (opt-in, DESIGN.md sections 22 and 28; pools of up to 64 slots on the HIP backend): the step streams FP8 e4m3fn copies of the dense weights (half
the bytes; the copies sit beside the bf16 weights, which the prefills keep reading).  `stats["weight_dtype"]` and
`stats["decode_weight_bytes"]` report the format and what a step streams.  It composes with every option above, `share_prompt_kv` and
`beam_search` included (every cache of a pool is built by `_new_caches`, which sets the step flags): only the dense launches of the step change.

`kv_paged=True` (opt-in): the KV cache is a pool of pages of `kv_page_tokens` tokens (`PagedKV`) and ONE device table
[n_slots, table_width] for all layers.  A job reserves ceil((prompt + its own limit) / page_tokens) pages from a host free list when it is
admitted -- nothing is allocated per step, so the captured step never waits for the host -- and returns them when its slot is fetched; its
table row then holds zeros again, the scrap page 0 that idle slots append into.  Without `kv_budget_tokens` the pool is sized per call for
the `n_slots` largest jobs; with it a free slot takes the head of the queue only when enough pages are free (FIFO: the head blocks the
jobs behind it; `stats["kv_page_waits"]` counts the slot-steps this idles), and a job larger than the whole budget is a ValueError.  The
step appends with `rope_append_decode_paged` and attends with `attention_decode_paged`.  Not with `share_prompt_kv` or `kv_dtype="fp8"`.

`batch_invariant=True` (opt-in; pools of up to 64 slots): a job's tokens, recorded logits and `last_logprobs` depend on
the model, its prompt, its sampling arguments, the seed and its sample index -- not on `n_slots`, the slot it ran in, the other jobs of the
call, the cache capacity, `kv_paged` / `kv_page_tokens`, `poll_every` or `EVO_AMD_DECODE_GRAPH`.  The step then runs ONE launch sequence at
every slot count -- norm, row-invariant projection (csrc/gemv_inv.hip), Hyena step or rotary + append, decode attention with 32 splits,
row-invariant output projection, norm, row-invariant gate and l3, final norm, row-invariant unembedding -- and gives up the fused dot2
launches of 1-8 slots.  Refused (ValueError, each has row-count- or group-dependent arithmetic of its own): `n_slots` > 64,
`prefill_batch` > 1, `share_prompt_kv`, `kv_dtype="fp8"`, `weight_dtype="fp8"`, and `beam_search` on such a pool.

k-mer repeat control (opt-in): `generate(repeat=RepeatControl(...))` also takes the job-control path and puts ONE more
launch, `evo_repeat_rows_f32`, in front of its sampler launch.  Every job keeps the counts of the k-mers of its prompt and of what it has
generated; the launch folds the token the step is fed (`DecodePool.ids`: what the previous step drew) into them, subtracts a level from
the logit of every nucleotide that would complete a k-mer seen before, and -- with `end_fraction` -- ends a job once more than that
fraction of its tokens were such repeats (`last_finish` "repeat"; the job keeps all its tokens).  The sampler draws from the penalised
row, so the recorded logits and `last_logprobs` of such a run are the penalised ones (`score_sequences` on the output gives the model's
own).  `last_repeats` holds one (generated tokens folded, repeats among them) per job, read when the job is fetched: a job the sampler
ended (limit, stop rule, constraint) has its last token not yet folded, a job the rule ended has all of them.  Row-local and outside the
forward, it composes with everything the job-control path composes with.

Beam search: `beam_search(prompts, n_tokens, beam_width)` on a pool built with `share_prompt_kv=True` returns the
`beam_width` most likely continuations of every prompt.  A prompt owns a group of `beam_width` consecutive slots behind one store row; the
captured step is forward, `beam_select` (the group's W x 512 candidates ranked on the device; parents, tokens and scores written where the
next step reads them), `gather_rows` out to a scratch buffer and back (every record of a slot -- FIR history, modal state, the keys it has
generated -- moves to the slot that continues its hypothesis), advance.  The host walks the recorded back-pointers when a group is fetched.

How the file is laid out.  Refusals and every attribute's declaration are in `DecodePool.__init__`.  `_new_caches` is the
one constructor of a pool's caches; the three KV layouts (`_RowsKV`: contiguous bf16 / FP8 rows, `_PagedKV`, `_StoreKV`: the shared prompt
store) add their K/V tensors to it and answer the scheduler's six calls -- `size`, `need` / `can_admit`, `install`, `release`, `advance`,
`nbytes` -- so that the scheduler never asks which layout it runs on.  `_check_job` validates a call's prompts and arguments for `generate`,
its job-control path and `beam_search`.  `_run` is the one scheduling loop of `generate` (admit, step, look, fetch) for its three sampler
modes; `_run_beam` is the beam search's own loop over groups.  `_captured` is the one place a step is captured and replayed; `_step`,
`_step_sampled` and `_step_beam` go through it.
"""
from __future__ import annotations

import weakref
from collections import deque
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from .scoring import logits_to_logprobs, prepare_batch
from .backend import Backend
from .sh.cache import (Fp8KV, PagedKV, PromptStore, check_kv_dtype, check_page_tokens, check_rowinv_rows, check_weight_dtype,
                       check_weight_rows)
from .sh.model import capture_graph
from .constraints import TokenConstraint
from .sh.sample import (FINISH_CONSTRAINT, FINISH_DEAD_END, FINISH_LENGTH, FINISH_NAMES_REPEAT, FINISH_REPEAT, FINISH_STOP_TOKEN, RepeatControl,
                        allowed_mask, sample, stop_patterns)


def _kv_bytes(kvs) -> int:
    """Bytes held by KV tensors of any of the formats: what stats["kv_bytes"] reports."""
    return sum(kv.nbytes() if isinstance(kv, (Fp8KV, PagedKV)) else kv.numel() * kv.element_size() for kv in kvs)


class _RowsKV:
    """The KV layouts of a pool.  The scheduler talks to its layout through these calls alone and never asks which
    one it has: `size` (for a call's jobs), `need` / `can_admit` (what a job reserves; may the head of the queue be admitted now),
    `install` (a prompt's K/V, from row `row` of a prefill, into a slot), `release` (finished slots), `advance` (every position by one)
    and `nbytes`.  A layout is chosen once, in DecodePool.__init__; the tensors and host lists it manages are the pool's declared state.

    This one is the contiguous layout, and the base of the other two: `capacity` KV rows per slot and layer, bf16 tensors or `Fp8KV`."""
    name = "contiguous"                                               # InferenceParams.kv_layout

    def __init__(self, pool: "DecodePool"):
        # (no cycle: a dropped pool dies by reference count, at once.  Left to the cycle collector, its captured graph would be destroyed
        # whenever the collector runs -- in the middle of another pool's stream capture, which aborts the process)
        self.p = weakref.proxy(pool)

    def size(self, lens: Sequence[int], limits: Sequence[int], copies: int, rows: Optional[int] = None) -> None:
        self.allocate(max(lens) + max(limits))

    def allocate(self, capacity: int) -> None:
        """Pool-wide caches with `capacity` KV rows per slot (grown geometrically, outside any captured graph)."""
        p = self.p
        m, S, dev = p.model, p.n_slots, p.device
        if p.ipd is not None and capacity <= p.capacity:
            return
        capacity = max(capacity, 2 * p.capacity)
        old = p.ipd
        ipd = p._new_caches(capacity)
        H, hd, dt = m.num_heads, m.head_dim, m.embedding_layer.weight.dtype
        for i in m.attn_layer_idxs:
            prev = None if old is None else old["mha"].key_value_memory_dict[i]
            if p.kv_dtype == "fp8":
                kv = Fp8KV.zeros(S, capacity, H, hd, dev)
                if prev is not None:
                    kv.copy_rows_(slice(None), prev, slice(None), prev.shape[1])
            else:
                kv = torch.zeros(S, capacity, 2, H, hd, dtype=dt, device=dev)
                if prev is not None:
                    kv[:, : prev.shape[1]] = prev
            ipd["mha"].key_value_memory_dict[i] = kv
        p.ipd, p.capacity = ipd, capacity
        p.stats["kv_bytes"] = self.nbytes()

    def need(self, n_keys: int) -> int:
        """What a job of `n_keys` = prompt + own limit tokens reserves at admission (pages; nothing here)."""
        return 0

    def can_admit(self, need: int) -> bool:
        return True

    def install(self, slot: int, pi: int, tmp: dict, P: int, **kw) -> None:
        """Slot `slot` continues prompt `pi` from row `row` of the prefill's caches `tmp`; `need`: what the job reserves.  (Through the
        pool's own method: it adds the Hyena states, and it is the name tests and tools hook.)"""
        self.p._install(slot, tmp, P, **kw)

    def put(self, slot: int, tmp: dict, P: int, row: int, need: int = 0, prompt: Optional[int] = None) -> None:
        for i in self.p.model.attn_layer_idxs:
            dst, src = self.p.ipd["mha"].key_value_memory_dict[i], tmp["mha"].key_value_memory_dict[i]
            if isinstance(dst, Fp8KV):
                dst.copy_rows_(slot, src, row, P)                        # both tensors of the layer
            else:
                dst[slot, :P] = src[row, :P]

    def release(self, slots: Sequence[int]) -> None:
        pass

    def advance(self) -> None:
        """Every slot moves on by one token (idle slots drift harmlessly; fill() resets them)."""
        self.p.pos.add_(1)
        self.p.pos.clamp_(max=self.p.capacity - 1)

    def nbytes(self) -> int:
        return _kv_bytes(self.p.ipd["mha"].key_value_memory_dict.values())


class _PagedKV(_RowsKV):
    """kv_paged: pages of `page_tokens` tokens and ONE device table `pool.table` for all layers; the host free list
    `pool._free_pages` (page 0, the scrap page, is never on it) and the pages of each slot's job `pool._slot_pages`."""
    name = "paged"

    def need(self, n_keys: int) -> int:
        return -(-int(n_keys) // self.p.page_tokens)

    def can_admit(self, need: int) -> bool:
        return need <= len(self.p._free_pages)

    def size(self, lens, limits, copies, rows=None) -> None:
        """Page pool and table for one call: a job reserves to its OWN limit.  The table is as wide as the largest need; without a budget
        the pool holds the `n_slots` largest needs (admission never waits), with one it holds the budget.  Runs between calls, when no job
        is live: a larger pool is allocated afresh and nothing is copied; a wider table or a new pool drops the captured step (it is
        bound to their addresses)."""
        p = self.p
        m, S, dev, pt = p.model, p.n_slots, p.device, p.page_tokens
        needs = [self.need(P + n) for P, n in zip(lens, limits) for _ in range(int(copies))]
        width = max(needs)
        if p.budget_pages is not None:
            if width > p.budget_pages:
                raise ValueError(f"kv_paged: a job needs {width} pages of {pt} tokens, the budget kv_budget_tokens holds "
                                 f"{p.budget_pages}")
            n_pages = 1 + p.budget_pages
        else:
            n_pages = 1 + sum(sorted(needs, reverse=True)[:S])
        fresh = p.ipd is None
        if fresh:
            p.ipd = p._new_caches(0)
            p._slot_pages = [[] for _ in range(S)]
        mha = p.ipd["mha"]
        if p.table is None or p.table.shape[1] < width:
            p.table = torch.zeros(S, width, dtype=torch.int32, device=dev)
            for kv in mha.key_value_memory_dict.values():
                kv.table = p.table
            p._graph = None
        if fresh or n_pages > p.stats["kv_pages"]:
            dt = m.embedding_layer.weight.dtype
            for i in m.attn_layer_idxs:
                mha.key_value_memory_dict.pop(i, None)               # (let go of the old pool before the new one is made)
                mha.key_value_memory_dict[i] = PagedKV.zeros(n_pages, pt, m.num_heads, m.head_dim, p.table, dtype=dt)
            p._free_pages = list(range(n_pages - 1, 0, -1))          # popped from the end: page 1 first; page 0 stays out
            p.stats["kv_pages"] = n_pages
            p.stats["kv_bytes"] = self.nbytes()
            p._graph = None
        p.capacity = p.table.shape[1] * pt                           # the bound of a slot's position
        mha.max_seqlen = p.capacity

    def put(self, slot, tmp, P, row, need=0, prompt=None) -> None:
        # the job's reservation: `need` pages off the free list, named in its table row (outside the captured step, like all of this)
        p = self.p
        pages = [p._free_pages.pop() for _ in range(need)]
        p._slot_pages[slot] = pages
        ids = torch.tensor(pages, dtype=torch.int64, device=p.device)
        p.table[slot, :need] = ids.to(torch.int32)
        p.stats["kv_pages_peak"] = max(p.stats["kv_pages_peak"], p.stats["kv_pages"] - 1 - len(p._free_pages))
        for i in p.model.attn_layer_idxs:                            # the prompt's K/V, from row `row` of the prefill's own cache
            p.ipd["mha"].key_value_memory_dict[i].write_tokens_(ids, tmp["mha"].key_value_memory_dict[i][row, :P])

    def release(self, slots) -> None:
        """Finished slots give their pages back; their table rows return to zeros (the scrap page)."""
        p = self.p
        for s in slots:
            p._free_pages.extend(reversed(p._slot_pages[s]))
            p._slot_pages[s] = []
        p.table[torch.tensor(list(slots), dtype=torch.int64, device=p.device)] = 0


class _StoreKV(_RowsKV):
    """share_prompt_kv: own caches of the generated tokens only, and `pool.store`, R rows of the longest prompt's
    length, each holding the K/V of one prompt for all its copies.  Host: `pool.store_refs` (live copies per row), `pool._store_prompt`
    (the prompt a row holds, kept after its last copy finished), `pool._slot_row` (mirror of store.row)."""

    def size(self, lens, limits, copies, rows=None) -> None:
        """Jobs run in order and have one length, so the live jobs are a window of at most S consecutive jobs: they touch at most
        ceil(S / n) + 1 prompts (and never more than S).  `rows`: jobs of unequal length break the window -- job 0 may outlive jobs
        1 ... 40 -- so the caller asks for min(S, number of prompts) rows: one per live slot, or one per prompt (beam: one per group)."""
        p = self.p
        m, S, dev = p.model, p.n_slots, p.device
        p_max, n_tokens = max(lens), max(limits)
        R = min(S, -(-S // int(copies)) + 1) if rows is None else int(rows)
        if p.store is not None and p.capacity >= n_tokens and p.store_cap >= p_max and len(p.store_refs) >= R:
            p._store_prompt = [None] * len(p.store_refs)             # prompt indices belong to one job list
            return
        ipd = p._new_caches(n_tokens)
        H, hd, dt = m.num_heads, m.head_dim, m.embedding_layer.weight.dtype
        st = PromptStore(row=torch.full((S,), -1, dtype=torch.int64, device=dev), length=torch.ones(R, dtype=torch.int64, device=dev),
                         own_pos=torch.zeros(S, dtype=torch.int64, device=dev))
        for i in m.attn_layer_idxs:
            ipd["mha"].key_value_memory_dict[i] = torch.zeros(S, n_tokens, 2, H, hd, dtype=dt, device=dev)
            st.kv[i] = torch.zeros(R, p_max, 2, H, hd, dtype=dt, device=dev)
        ipd["mha"].prompt_store = st
        p.ipd, p.capacity, p.store, p.store_cap = ipd, n_tokens, st, p_max
        p.store_refs, p._store_prompt, p._slot_row = [0] * R, [None] * R, [-1] * S
        p.stats["store_rows"] = R
        p.stats["kv_bytes"] = self.nbytes()

    def install(self, slot, pi, tmp, P, **kw) -> None:
        self.p._install_shared(slot, pi, tmp, P, **kw)

    def put(self, slot, tmp, P, row, need=0, prompt=None) -> None:
        """The prompt's K/V goes into a store row unless one holds it already."""
        p, st = self.p, self.p.store
        if prompt in p._store_prompt:
            r = p._store_prompt.index(prompt)
        else:
            r = p.store_refs.index(0)                                # (exists: see size)
            for i in p.model.attn_layer_idxs:
                st.kv[i][r, :P] = tmp["mha"].key_value_memory_dict[i][row, :P]
            st.length[r] = P
            p._store_prompt[r] = prompt
            p.stats["prompt_kv_installs"] += 1
        p.store_refs[r] += 1
        p._slot_row[slot] = r
        st.row[slot] = r
        st.own_pos[slot] = 0

    def release(self, slots) -> None:
        """Finished slots let go of their store rows (the host knows when: it fetches them) and point at none."""
        p = self.p
        for s in slots:
            p.store_refs[p._slot_row[s]] -= 1
            p._slot_row[s] = -1
        p.store.row[torch.tensor(list(slots), dtype=torch.int64, device=p.device)] = -1

    def advance(self) -> None:
        p = self.p
        p.pos.add_(1)
        p.pos.clamp_(max=p.store_cap + p.capacity - 1)
        p.store.own_pos.add_(1)
        p.store.own_pos.clamp_(max=p.capacity - 1)

    def nbytes(self) -> int:
        return _kv_bytes(list(self.p.ipd["mha"].key_value_memory_dict.values()) + list(self.p.store.kv.values()))


class DecodePool:
    # options that do not combine (ValueError), in the order they are refused: (one option, the other, the message)
    _EXCLUSIVE = (
        ("batch_invariant", "prefill_batch", "batch_invariant=True does not combine with prefill_batch > 1 (a padded batch's prefill depends on "
                                             "the prompts admitted together)"),
        ("batch_invariant", "share_prompt_kv", "batch_invariant=True does not combine with share_prompt_kv=True (the grouped decode attention "
                                               "splits by group)"),
        ("batch_invariant", "kv_fp8", 'batch_invariant=True does not combine with kv_dtype="fp8"'),
        ("batch_invariant", "w_fp8", 'batch_invariant=True does not combine with weight_dtype="fp8"'),
        ("kv_paged", "share_prompt_kv", "kv_paged=True does not combine with share_prompt_kv=True: the prompt store and its grouped decode "
                                        "attention read contiguous rows"),
        ("kv_paged", "kv_fp8", 'kv_paged=True does not combine with kv_dtype="fp8": the paged cache and its two kernels are bf16'),
        ("kv_fp8", "share_prompt_kv", 'kv_dtype="fp8" does not combine with share_prompt_kv=True: the prompt store and its grouped decode '
                                      "attention are bf16"),
    )

    def __init__(self, model, tokenizer, n_slots: int = 8, top_k: int = 4, top_p: float = 1.0,
                 temperature: float = 0.7, device: Optional[str] = None, use_graph: Optional[bool] = None,
                 seed: Optional[int] = None, allowed_tokens=None, share_prompt_kv: bool = False, prefill_batch: int = 1,
                 prefill_max_tokens: int = 32768, poll_every: int = 8, kv_dtype: str = "bf16", weight_dtype: str = "bf16",
                 kv_paged: bool = False, kv_page_tokens: int = 256, kv_budget_tokens: Optional[int] = None, batch_invariant: bool = False):
        # every refusal before any device work (DESIGN.md sections 21-23, 25): values, then pairs of options, then what the backend lacks
        self.model = model
        self.kv_dtype, self.weight_dtype = check_kv_dtype(kv_dtype), check_weight_dtype(weight_dtype)
        self.batch_invariant, self.kv_paged, self.share_prompt_kv = bool(batch_invariant), bool(kv_paged), bool(share_prompt_kv)
        self.poll_every, self.prefill_batch, self.prefill_max_tokens = int(poll_every), int(prefill_batch), int(prefill_max_tokens)
        if self.batch_invariant:
            check_rowinv_rows(int(n_slots), "n_slots")
        on = {"batch_invariant": self.batch_invariant, "kv_paged": self.kv_paged, "share_prompt_kv": self.share_prompt_kv,
              "prefill_batch": self.prefill_batch > 1, "kv_fp8": self.kv_dtype != "bf16", "w_fp8": self.weight_dtype != "bf16"}
        for a, b, message in self._EXCLUSIVE:
            if on[a] and on[b]:
                raise ValueError(message)
        self.page_tokens = self.budget_pages = None
        if self.kv_paged:
            self.page_tokens = check_page_tokens(kv_page_tokens)
            if kv_budget_tokens is not None:
                self.budget_pages = int(kv_budget_tokens) // self.page_tokens
                if self.budget_pages < 1:
                    raise ValueError(f"kv_budget_tokens = {kv_budget_tokens} holds no page of {self.page_tokens} tokens")
        if self.weight_dtype == "fp8":                               # 
            from .generation import check_fp8_weight_model, w8_rows
            check_weight_rows(int(n_slots), "n_slots", w8_rows(model))
            check_fp8_weight_model(model, int(n_slots))
        if self.poll_every < 1:
            raise ValueError("poll_every must be >= 1")
        if self.prefill_batch < 1:
            raise ValueError("prefill_batch must be >= 1")
        if self.prefill_batch > 1 and not hasattr(model, "prefill_ragged"):
            raise RuntimeError("prefill_batch > 1 needs a model with prefill_ragged (one forward over prompts of unequal length)")
        ops = getattr(model, "ops", None)

        def has(*groups):
            return ops is not None and Backend.adopt(ops).supports(*groups)
        for wanted, option, kernels, there in (
                (self.batch_invariant, "batch_invariant=True", 'the "row_invariant" kernels (' + ", ".join(Backend.OPTIONAL["row_invariant"])
                 + ") and hyena_step", lambda: has("row_invariant", "hyena_step")),
                (self.kv_paged, "kv_paged=True", 'the "kv_paged" kernels (rope_append_decode_paged, attention_decode_paged)', lambda: has("kv_paged")),
                (self.share_prompt_kv, "share_prompt_kv=True", "attention_decode_prefix (the decode attention over a shared prompt store)",
                 lambda: hasattr(ops, "attention_decode_prefix")),
                (self.kv_dtype == "fp8", 'kv_dtype="fp8"', 'the "kv_fp8" kernels (kv_quant_fp8, rope_append_decode_fp8, attention_decode_fp8)',
                 lambda: has("kv_fp8"))):
            if wanted and not there():
                raise RuntimeError(f"{option} needs a compute backend with {kernels}; this model's backend has none")
        self.tok = tokenizer
        self.n_slots = int(n_slots)
        self.top_k, self.top_p, self.temperature = top_k, top_p, temperature
        self.device = torch.device(device) if device is not None else model.device
        self.use_graph = (self.device.type == "cuda" and getattr(model, "decode_graph", False)) \
            if use_graph is None else bool(use_graph)
        self.stats = {"steps": 0, "prefills": 0, "tokens": 0, "batch_invariant": self.batch_invariant}
        if hasattr(model, "decode_weight_bytes"):
            self.stats.update({"weight_dtype": self.weight_dtype, "decode_weight_bytes": model.decode_weight_bytes(self.weight_dtype)})
        if self.share_prompt_kv:
            self.stats.update({"prompt_kv_installs": 0, "store_rows": 0, "prefix_streams": 0})
        if self.prefill_batch > 1:                                   # (prefills then counts forwards)
            self.stats.update({"prefill_prompts": 0, "prefill_pad_tokens": 0})
        if self.kv_paged:
            self.stats.update({"kv_pages": 0, "kv_pages_peak": 0, "kv_page_waits": 0})
        # the KV layout, chosen once: from here on nothing asks which one the pool has
        self.kv = (_StoreKV if self.share_prompt_kv else _PagedKV if self.kv_paged else _RowsKV)(self)
        # all state is declared here; the layout and the allocators below fill it in
        self.ipd = None
        self.capacity = 0
        self.pos = self.ids = None                                   # device: every slot's position [S] and the token it is fed [S, 1]
        self.table = None                                            # kv_paged: device int32 [S, table_width], shared by every layer's PagedKV
        self._free_pages: List[int] = []                             # host free list (page 0, the scrap page, is never on it)
        self._slot_pages: List[List[int]] = []                       # host: the pages each slot's job owns
        self.store = None
        self.store_cap = 0                                           # share_prompt_kv: the keys a store row holds
        self.store_refs: List[int] = []                              # host: live copies per store row
        self._store_prompt: List[Optional[int]] = []                 # host: the prompt a store row holds (kept after its last copy finished)
        self._slot_row: List[int] = []                               # host mirror of store.row
        # seeded / restricted sampling runs on the device; with neither the host sampler of the reference stays (the default)
        self.device_sampler = seed is not None or allowed_tokens is not None
        self.seed = 0 if seed is None else int(seed)
        self.allow_mask = None if allowed_tokens is None else allowed_mask(tokenizer, allowed_tokens)
        # per-slot sampler state (_allocate_sampler_state), the automata table (_upload_constraints), repeat-control state (_allocate_repeat)
        self.s_top_k = self.s_top_p = self.s_temperature = self.s_stream = self.s_count = self.s_active = self.s_logprob = None
        self.s_allow = self.s_stop_mask = self.s_limit = self.s_length = self.s_finish = self.s_dfa_base = self.s_dfa_state = None
        self.s_dfa_next = None
        self.s_rep_counts = self.s_rep_ctx = self.s_rep_stat = self.s_rep_levels = self.s_rep_end = self.s_rep_logits = None
        self.hist_ids = self.hist_logits = self.hist_logprob = None
        self._graph = None                                           # the captured step: (graph, its output tensor or None)
        self._ctl = None                                             # job control: the stop rule of the running generate()
        self._graph_key = None                                       # what the captured step's sampler launch was captured with
        self._beam = self._beam_graph = None                         # beam search: its state and its captured step

    # ------------------------------------------------------------------ caches
    def _new_caches(self, max_seqlen: int) -> dict:
        """The one constructor of a pool's caches: the `ipd` pair with every step flag set from the pool's options, the Hyena FIR and modal
        states, `pos`, `ids` and (with the device sampler) the sampler state.  The layout adds its K/V tensors and keeps the result.  New
        caches drop the captured step."""
        m, S, dev = self.model, self.n_slots, self.device
        ipd = m.initialize_inference_params()
        mha = ipd["mha"]
        mha.max_batch_size = ipd["hyena"].max_batch_size = S
        mha.max_seqlen = max_seqlen
        mha.kv_dtype, mha.kv_layout, mha.batch_invariant = self.kv_dtype, self.kv.name, self.batch_invariant
        mha.weight_dtype = self.weight_dtype                         # (the steps; a prefill runs on a cache of its own and reads bf16 weights)
        D, dt = m.hidden_size, m.embedding_layer.weight.dtype
        for i in m.hyena_layer_idxs:
            ipd["hyena"].fir_state_dict[i] = torch.zeros(S, 3 * D, m.short_filter_length - 1, dtype=dt, device=dev)
            ipd["hyena"].state_dict[i] = torch.zeros(S, D, m.state_size, dtype=torch.complex64, device=dev)
        self.pos = torch.zeros(S, dtype=torch.int64, device=dev)
        self.ids = torch.zeros(S, 1, dtype=torch.int64, device=dev)
        if self.device_sampler:
            self._allocate_sampler_state()
        self._graph = None
        return ipd

    def _allocate(self, capacity: int) -> None:
        """Contiguous caches with at least `capacity` KV rows per slot (the layout's own allocator, under the name it always had)."""
        self.kv.allocate(capacity)

    def _install(self, slot: int, tmp: dict, P: int, row: int = 0, need: int = 0) -> None:
        """Row `row` of a prefill's caches `tmp` into slot `slot`: the prompt's K/V by the layout (`need`: the pages the job reserves), the
        Hyena states per slot."""
        self.kv.put(slot, tmp, P, row, need=need)
        self._install_states(slot, tmp, row)

    def _install_shared(self, slot: int, pi: int, tmp: dict, P: int, row: int = 0) -> None:
        """The same for a layout that holds a prompt's K/V once for all its copies: slot `slot` continues prompt `pi`."""
        self.kv.put(slot, tmp, P, row, prompt=pi)
        self._install_states(slot, tmp, row)

    def _install_states(self, slot: int, tmp: dict, row: int) -> None:
        for i in self.model.hyena_layer_idxs:
            self.ipd["hyena"].fir_state_dict[i][slot] = tmp["hyena"].fir_state_dict[i][row]
            self.ipd["hyena"].state_dict[i][slot] = tmp["hyena"].state_dict[i][row].reshape(
                self.ipd["hyena"].state_dict[i][slot].shape)

    def _count_prefix_streams(self) -> None:
        """The store rows one step streams: per workgroup tile of the grouped kernel, the distinct rows among its slots."""
        gr = int(self.model.ops.attn_group_rows)
        self.stats["prefix_streams"] += sum(len({r for r in self._slot_row[t:t + gr] if r >= 0}) for t in range(0, self.n_slots, gr))

    def _allocate_sampler_state(self) -> None:
        m, S, dev = self.model, self.n_slots, self.device
        # per-slot sampler state, all of it read by the captured launch
        self.s_top_k = torch.full((S,), int(self.top_k), dtype=torch.int32, device=dev)
        self.s_top_p = torch.full((S,), float(self.top_p), dtype=torch.float32, device=dev)
        self.s_temperature = torch.full((S,), float(self.temperature), dtype=torch.float32, device=dev)
        self.s_stream = torch.zeros(S, dtype=torch.int64, device=dev)
        self.s_count = torch.zeros(S, dtype=torch.int64, device=dev)
        self.s_active = torch.zeros(S, dtype=torch.bool, device=dev)
        self.s_logprob = torch.zeros(S, dtype=torch.float32, device=dev)
        self.s_allow = None if self.allow_mask is None else m.ops.pack_allow_mask(self.allow_mask, dev)
        self.s_stop_mask = torch.zeros(64, dtype=torch.uint8, device=dev)     # the stop tokens of the running rule: a captured launch keeps this address
        self.hist_ids = self.hist_logits = self.hist_logprob = None
        # job control: limit in, length (-1 while the job runs) and finish out
        self.s_limit = torch.zeros(S, dtype=torch.int64, device=dev)
        self.s_length = torch.full((S,), -1, dtype=torch.int64, device=dev)
        self.s_finish = torch.zeros(S, dtype=torch.uint8, device=dev)
        # constrained generation: the table row of the slot's state 0 (-1: the slot's job is free) and its state relative to that row
        self.s_dfa_base = torch.full((S,), -1, dtype=torch.int64, device=dev)
        self.s_dfa_state = torch.zeros(S, dtype=torch.int32, device=dev)

    def _allocate_history(self, n_tokens: int) -> None:
        """Device-resident record of every slot's current job: tokens [S, L] and the f32 logits that produced them [S, L, V]."""
        if self.hist_ids is not None and self.hist_logits is not None and self.hist_ids.shape[1] >= n_tokens:
            return
        S, dev = self.n_slots, self.device
        self.hist_logprob = None
        self.hist_ids = torch.zeros(S, n_tokens, dtype=torch.int64, device=dev)
        self.hist_logits = torch.zeros(S, n_tokens, self.model.vocab_size, dtype=torch.float32, device=dev)
        self._graph = None

    def _prefill(self, ids: torch.Tensor, logits_dtype=torch.float32):
        """ids [1, P] -> (last-position logits [V] f32, the B = 1 caches of the prompt)."""
        m = self.model
        tmp = m.initialize_inference_params()
        tmp["mha"].max_seqlen = ids.shape[1]
        tmp["mha"].kv_dtype = self.kv_dtype
        with torch.inference_mode():
            logits, tmp = m(ids, inference_params_dict=tmp)
        self.stats["prefills"] += 1
        return logits[0, -1].to(logits_dtype), tmp

    # ------------------------------------------------------------------ prompts admitted together share one prefill (opt-in)
    PREFILL_PAD = 64                                                   # StripedHyena.prefill_ragged's pad_to

    def _prefill_group(self, window: Sequence[int], lengths: Sequence[int]) -> List[int]:
        """The admission rule of `prefill_batch` > 1.  `window`: the prompt index of every job the currently idle slots will take, in job
        order (the first one is the prompt that needs a prefill now).  Taken: the distinct prompts in that order, at most `prefill_batch`,
        stopping before (prompts) x (longest length, rounded up to PREFILL_PAD) exceeds `prefill_max_tokens`.  A single prompt -- nothing
        to share with, or alone beyond the cap -- is returned alone: it goes through the B = 1 prefill unchanged."""
        group: List[int] = []
        t_max = 0
        for pi in window:
            if pi in group:
                continue
            if len(group) == self.prefill_batch:
                break
            t = max(t_max, -(-int(lengths[pi]) // self.PREFILL_PAD) * self.PREFILL_PAD)
            if group and (len(group) + 1) * t > self.prefill_max_tokens:
                break
            group.append(pi)
            t_max = t
        return group

    def _prefill_ragged(self, encoded: Sequence[torch.Tensor], group: Sequence[int], logits_dtype=torch.float32):
        """The prompts `group` in ONE forward -> (last-position logits [B, V] f32, the caches of the padded batch: row b = group[b])."""
        lens = [int(encoded[pi].shape[1]) for pi in group]
        T = max(lens)
        ids = torch.stack([torch.cat([encoded[pi][0], encoded[pi][0, -1:].expand(T - n)]) for pi, n in zip(group, lens)])
        with torch.inference_mode():
            fp8 = {} if self.kv_dtype == "bf16" else {"kv_dtype": self.kv_dtype}
            logits, tmp = self.model.prefill_ragged(ids, lens, pad_to=self.PREFILL_PAD, **fp8)
        self.stats["prefills"] += 1
        self.stats["prefill_pad_tokens"] += len(group) * (-(-T // self.PREFILL_PAD) * self.PREFILL_PAD) - sum(lens)
        return logits.to(logits_dtype), tmp

    # ------------------------------------------------------------------ one token for every slot
    def _step_eager(self) -> torch.Tensor:
        m, mha = self.model, self.ipd["mha"]
        mha.pos_tensor = self.pos
        try:
            h = m.hidden_states(self.ids, self.ipd)
            unembed = m.ops.linear_rowinv if self.batch_invariant else m.ops.linear
            return unembed(h, m.unembed.weight, None).view(self.n_slots, m.vocab_size)
        finally:
            mha.pos_tensor = None

    def _captured(self, held, eager):
        """One step under `use_graph`: `eager` is the step, `held` its captured form (graph, output) or None -> (what the step returned --
        the eager run's tensor, or the one the replay writes --, the captured form to keep)."""
        with torch.inference_mode():
            if not self.use_graph:
                return eager(), None
            if held is None:
                # The first step runs eagerly (it also warms the library handles and the M = S GEMM choices) and IS the
                # step: the caches advance in place, so nothing may run twice.  Capture records without executing.
                first = eager()
                torch.cuda.synchronize(self.device)
                self.model._row_index(self.n_slots, self.device)
                g = torch.cuda.CUDAGraph()
                with capture_graph(g):
                    out = eager()
                return first, (g, out)
            held[0].replay()
            return held[1], held

    def _step(self) -> torch.Tensor:
        """self.ids [S,1] at positions self.pos [S] -> logits [S, V] f32 (every slot, active or not)."""
        self.stats["steps"] += 1
        with torch.inference_mode():
            logits, self._graph = self._captured(self._graph, self._step_eager)
            return logits.float()

    # ------------------------------------------------------------------ the same step with the sampler as its last node
    def _sample_rows(self, logits: torch.Tensor, rows: slice, active) -> None:
        self.model.ops.sample_rows(logits, self.s_top_k[rows], self.s_top_p[rows], self.s_temperature[rows], self.seed,
                                   stream=self.s_stream[rows], count=self.s_count[rows], allow=self.s_allow, active=active,
                                   ids_out=self.ids[rows], logprob_out=self.s_logprob[rows], hist_ids=self.hist_ids[rows],
                                   hist_logits=self.hist_logits[rows])

    def _sample_rows_ctl(self, logits: torch.Tensor, rows: slice) -> None:
        """The sampler launch of the job-control path: the same draw, and a row that ends its job clears its own `s_active`."""
        c = self._ctl
        launch, dfa = self.model.ops.sample_rows_ctl, {}
        if c["dfa"] is not None:                                     # constrained generation: the same launch under the slots' automata
            launch = self.model.ops.sample_rows_dfa
            dfa = dict(dfa_alphabet=c["dfa"]["alphabet"], dfa_next=c["dfa"]["next"], dfa_base=self.s_dfa_base[rows],
                       dfa_state=self.s_dfa_state[rows])
        launch(logits, self.s_top_k[rows], self.s_top_p[rows], self.s_temperature[rows], self.seed,
               count=self.s_count[rows], active=self.s_active[rows], limit=self.s_limit[rows],
               length=self.s_length[rows], finish=self.s_finish[rows], stream=self.s_stream[rows],
               allow=self.s_allow, ids_out=self.ids[rows], logprob_out=self.s_logprob[rows],
               hist_ids=self.hist_ids[rows], hist_logits=None if self.hist_logits is None else self.hist_logits[rows],
               hist_logprob=self.hist_logprob[rows], stop_mask=c["stop_mask"], stop_seq=c["stop_seq"],
               stop_frame=c["stop_frame"], **dfa)

    # ------------------------------------------------------------------ k-mer repeat control (opt-in)
    def _allocate_repeat(self, rc) -> None:
        """Per-pool state of the repeat launch: counts [S, M] (4 M bytes per slot; 4 MiB at the cap M = 2^20), window, statistics, levels, the
        armed fraction, and the f32 rows the sampler reads.  A new table size makes new state and drops the captured step."""
        S, dev = self.n_slots, self.device
        if self.s_rep_counts is not None and tuple(self.s_rep_counts.shape) == (S, rc.M):
            return
        self.s_rep_counts = torch.zeros(S, rc.M, dtype=torch.int32, device=dev)
        self.s_rep_ctx = torch.zeros(S, 2, dtype=torch.int32, device=dev)
        self.s_rep_stat = torch.zeros(S, 2, dtype=torch.int64, device=dev)
        self.s_rep_levels = torch.zeros(S, 8, dtype=torch.float32, device=dev)
        self.s_rep_end = torch.zeros(S, dtype=torch.int32, device=dev)
        self.s_rep_logits = torch.zeros(S, self.model.vocab_size, dtype=torch.float32, device=dev)
        self._graph = None

    def _repeat_init(self, ids: torch.Tensor, rc) -> Tuple[torch.Tensor, torch.Tensor]:
        """`repeat_init` (sh/sample.py) of one prompt with torch ops on the pool's device, outside the captured step: ids [P] -> (counts [M]
        int32, (code, len) int32 [2]).  A k-mer counts when its k tokens are consecutive alphabet symbols; the window is the last
        min(k - 1, trailing run of symbols) of them."""
        dev, n, k = ids.device, rc.n_sym, rc.k
        lut = torch.full((512,), -1, dtype=torch.int64, device=dev)
        lut[torch.tensor(rc.ids, dtype=torch.int64, device=dev)] = torch.arange(n, dtype=torch.int64, device=dev)
        ids = ids.reshape(-1).to(torch.int64)
        inside = (ids >= 0) & (ids < 512)
        sym = torch.where(inside, lut[ids.clamp(0, 511)], torch.full_like(ids, -1))
        P = int(sym.numel())
        counts = torch.zeros(rc.M, dtype=torch.int64, device=dev)
        if rc.count_prompt and P >= k:
            w = sym.unfold(0, k, 1)                                   # [P - k + 1, k], oldest symbol first
            ok = (w >= 0).all(-1)
            place = n ** torch.arange(k - 1, -1, -1, dtype=torch.int64, device=dev) if n > 1 else torch.zeros(k, dtype=torch.int64, device=dev)
            counts = torch.bincount((w.clamp(min=0) * place).sum(-1)[ok], minlength=rc.M)
        tail = sym[max(0, P - (k - 1)):].tolist() if k > 1 else []
        code = ln = 0
        for a in tail:                                                # at most k - 1 <= 19 symbols (n_sym = 1: the code stays 0)
            code, ln = (0, 0) if a < 0 else (code * n + a, ln + 1)
        return counts.clamp(max=2 ** 31 - 1).to(torch.int32), torch.tensor([code, ln], dtype=torch.int32, device=dev)

    def _repeat_rows(self, logits: torch.Tensor, rows: slice, fed: bool) -> None:
        """The repeat launch on the slots `rows`: model rows in, `s_rep_logits[rows]` out.  `fed`: fold `self.ids`, the token the step is fed."""
        r = self._ctl["repeat"]
        end = dict(end_num=self.s_rep_end[rows], end_min_tokens=r["end_min_tokens"], count=self.s_count[rows], length=self.s_length[rows],
                   finish=self.s_finish[rows]) if r["armed"] else {}
        self.model.ops.repeat_rows(logits, self.s_rep_logits[rows], self.s_active[rows], self.s_rep_counts[rows], self.s_rep_ctx[rows],
                                   self.s_rep_stat[rows], self.s_rep_levels[rows], r["alphabet"], r["k"],
                                   fed_ids=self.ids[rows] if fed else None, **end)


    def _step_sample_eager(self) -> None:
        if self._ctl is not None:
            logits = self._step_eager()
            if self._ctl["repeat"] is not None:                      # self.ids still holds the token this step was fed
                self._repeat_rows(logits, slice(0, self.n_slots), fed=True)
                logits = self.s_rep_logits
            self._sample_rows_ctl(logits, slice(0, self.n_slots))
        else:
            self._sample_rows(self._step_eager(), slice(0, self.n_slots), self.s_active)     # bf16 logits, next ids -> self.ids
        self.kv.advance()

    def _step_sampled(self) -> None:
        """One token for every active slot, nothing returned to the host: ids, counters and history advance on the device."""
        self.stats["steps"] += 1
        _, self._graph = self._captured(self._graph, self._step_sample_eager)

    def _prefill_for(self, pi: int, jobs, slot_job, encoded, cached_prefill: Dict[int, tuple], logits_dtype=torch.float32) -> None:
        """Prompt `pi` needs a prefill: it, and with `prefill_batch` > 1 the prompts admitted with it, land in `cached_prefill` as
        (last-position logits [V] f32, caches, row of those caches)."""
        cached_prefill.clear()                               # keep one prefill's caches alive at a time (every earlier prompt's copies are installed)
        group = [pi]
        if self.prefill_batch > 1:
            # the jobs the idle slots (this one included) will take: copies of a prompt are adjacent, so none of them has a prefill yet
            n_idle = sum(1 for q in slot_job if q is None)
            group = self._prefill_group([pi] + [jobs[k][1] for k in range(min(n_idle - 1, len(jobs)))],
                                        [e.shape[1] for e in encoded])
            self.stats["prefill_prompts"] += len(group)
        if len(group) == 1:
            cached_prefill[pi] = self._prefill(encoded[pi], logits_dtype) + (0,)
        else:
            lg, tmp_b = self._prefill_ragged(encoded, group, logits_dtype)
            for r, q in enumerate(group):
                cached_prefill[q] = (lg[r], tmp_b, r)

    # ------------------------------------------------------------------ the job
    def generate(self, prompts: Sequence[str], n_tokens=1000, n_sample_per_prompt: int = 1,
                 prepend_bos: bool = False, sampling: Optional[Sequence[Optional[dict]]] = None,
                 streams: Optional[Sequence[int]] = None, stop_tokens=None, stop_sequences=None, stop_frame: int = 1,
                 return_logits: bool = True, constraints=None, repeat: Optional[RepeatControl] = None) \
            -> Tuple[List[str], List[float], List[int]]:
        """Returns (generated strings, mean log-likelihood scores, index of the prompt each came from), in job
        order: prompt 0's samples first.  `sampling` (device sampler only): one dict of `top_k` / `top_p` / `temperature`
        per prompt (or None) overriding the pool's own settings for that prompt's samples; `streams`: the random-stream id of
        every output (default: its index, `prompt index * n_sample_per_prompt + copy`), for a job that is a re-ordered part of another.

        Job control (any of these moves the sampler onto the device, seed 0 without a seed): `n_tokens` as a sequence
        is one length limit per prompt; `stop_tokens` (ids, or a string through the tokenizer) end a job and are trimmed from its string;
        `stop_sequences` (strings or id lists, at most 8 of 1 to 8 tokens) end it when they end at a multiple of `stop_frame` tokens,
        counted from the first generated one, and stay in its string; `return_logits=False` keeps no logits at all.  The run leaves
        `last_lengths`, `last_finish` ("stop_token" | "stop_sequence" | "length"), `last_logprobs`; `last_ids` holds -1 beyond a job's length.

        Constrained generation (also on the job-control path): `constraints` is one `TokenConstraint` for every prompt, or
        a list with one (or None: that prompt is free) per prompt.  It governs the GENERATED tokens: every sample starts in state 0, the
        prompt is not walked.  A job ends with the token that completes its constraint (`last_finish` "constraint", kept in its string).

        k-mer repeat control (also on the job-control path): `repeat` is one `RepeatControl` for the call.  The sampler
        then draws from rows with a level subtracted on every symbol that would complete a k-mer the job has seen (its prompt's included,
        unless `count_prompt=False`); the recorded logits and `last_logprobs` are those penalised rows.  With `end_fraction` a job ends
        (`last_finish` "repeat", all its tokens kept) once more than that fraction of its generated tokens were repeats.  `last_repeats`:
        one (n_gen, rep) per job -- the generated tokens folded into its counts and the repeats among them; the last token of a job the
        sampler ended is not folded, every token of a job the rule ended is."""
        m, tok, S, dev = self.model, self.tok, self.n_slots, self.device
        ctl = (not isinstance(n_tokens, (int, np.integer)) or stop_tokens is not None or stop_sequences is not None or int(stop_frame) != 1
               or not return_logits or constraints is not None or repeat is not None)
        if hasattr(m, "eval"):
            m.eval()
        n_spp = int(n_sample_per_prompt)
        prompts, limits, sampling = self._check_job(prompts, n_tokens, n_spp, prepend_bos, sampling, streams, ctl=ctl)
        if ctl:
            return self._generate_ctl(prompts, limits, n_spp, prepend_bos, sampling, streams, stop_tokens, stop_sequences, stop_frame,
                                      return_logits, constraints, repeat)
        if self._graph_key is not None:                              # the captured step ends with the job-control launch: capture anew
            self._graph, self._graph_key, self._ctl = None, None, None
        if not prompts:
            return [], [], []
        encoded = [prepare_batch([p], tok, prepend_bos=prepend_bos, device=str(dev))[0] for p in prompts]
        self.kv.size([e.shape[1] for e in encoded], limits, n_spp)
        if self.device_sampler:
            self._allocate_history(limits[0])
        return self._run("rows" if self.device_sampler else "host", prompts, encoded, limits, n_spp, sampling, streams)

    def _check_job(self, prompts, n_tokens, n_spp: int = 1, prepend_bos: bool = False, sampling=None, streams=None, ctl: bool = False,
                   beam: bool = False):
        """The one validation of a call's jobs, before any device work -> (prompts as a list, one limit per prompt, `sampling` as a list).
        `ctl`: the job-control path (its sampler is the device's whatever the pool's own is); `beam`: beam_search (an empty list is an
        error there, and there is no n_sample_per_prompt to name)."""
        prompts = list(prompts)
        one = isinstance(n_tokens, (int, np.integer))
        limits = [int(n_tokens)] * len(prompts) if one else [int(n) for n in n_tokens]
        if len(limits) != len(prompts):
            raise ValueError("n_tokens: one limit, or one per prompt")
        if (one and int(n_tokens) < 1) or any(n < 1 for n in limits) or n_spp < 1:
            raise ValueError("n_tokens must be >= 1" if beam else "n_tokens and n_sample_per_prompt must be >= 1")
        if beam and not prompts:
            raise ValueError("beam_search: the prompt list is empty")
        if any((not isinstance(p, str)) or (len(p) == 0 and not prepend_bos) for p in prompts):
            raise ValueError("every prompt must be a non-empty string (or use prepend_bos=True)")
        device = self.device_sampler or ctl
        if sampling is not None and prompts:
            if not device:
                raise ValueError("per-prompt sampling settings need the device sampler (give the pool a seed)")
            sampling = list(sampling)
            if len(sampling) != len(prompts) or any(d is not None and set(d) - {"top_k", "top_p", "temperature"} for d in sampling):
                raise ValueError("sampling: one dict of top_k / top_p / temperature (or None) per prompt")
        if streams is not None and prompts and (not device or len(streams) != len(prompts) * n_spp):
            raise ValueError("streams: one id per output" + ("" if ctl else ", and only with the device sampler"))
        return prompts, limits, sampling


    # ------------------------------------------------------------------ the job, with jobs that end on their own
    def _allocate_history_ctl(self, n_tokens: int, return_logits: bool) -> None:
        """Tokens [S, L] and their log-probabilities [S, L] on the device; the f32 logits [S, L, V] only when they are asked for."""
        S, dev = self.n_slots, self.device
        if self.hist_ids is None or self.hist_ids.shape[1] < n_tokens:
            self.hist_ids = torch.zeros(S, n_tokens, dtype=torch.int64, device=dev)
            self.hist_logits = self.hist_logprob = None
            self._graph = None
        L = self.hist_ids.shape[1]
        if self.hist_logprob is None:
            self.hist_logprob = torch.zeros(S, L, dtype=torch.float32, device=dev)
            self._graph = None
        if not return_logits:
            if self.hist_logits is not None:
                self.hist_logits = None                              # (an earlier job's: this one records none)
                self._graph = None
        elif self.hist_logits is None:
            self.hist_logits = torch.zeros(S, L, self.model.vocab_size, dtype=torch.float32, device=dev)
            self._graph = None

    def _constraints_of(self, constraints, n_prompts: int):
        """`constraints` of generate() -> (one TokenConstraint or None per prompt, the distinct ones in order of first use).  Checked here,
        before any device work: every constraint against the pool's allowed tokens, and one alphabet for all of them."""
        per = [constraints] * n_prompts if isinstance(constraints, TokenConstraint) else list(constraints)
        if len(per) != n_prompts or any(c is not None and not isinstance(c, TokenConstraint) for c in per):
            raise ValueError("constraints: one TokenConstraint, or one (or None) per prompt")
        distinct: List[TokenConstraint] = []
        for c in per:
            if c is not None and not any(c is d for d in distinct):
                c.validate(self.allow_mask)
                distinct.append(c)
        if len({c.alphabet for c in distinct}) > 1:
            raise ValueError("constraints: all constraints of one call must share one alphabet")
        return per, distinct

    def _upload_constraints(self, per, distinct):
        """The distinct automata, concatenated once into ONE device table [total states, 8] (per-pool state: a table of the same size is
        copied into the one the captured launch reads) -> (what the launch takes, the table row of every prompt's state 0; -1: free)."""
        offsets, total = {}, 0
        for c in distinct:
            offsets[id(c)] = total
            total += c.n_states
        table = torch.from_numpy(np.concatenate([c.table for c in distinct]).astype(np.int32))
        if self.s_dfa_next is None or tuple(self.s_dfa_next.shape) != tuple(table.shape):
            self.s_dfa_next = table.to(self.device)
        else:
            self.s_dfa_next.copy_(table)
        bases = [-1 if c is None else offsets[id(c)] for c in per]
        return {"alphabet": torch.tensor(distinct[0].alphabet, dtype=torch.int32), "next": self.s_dfa_next}, bases


    def _generate_ctl(self, prompts, limits, n_spp, prepend_bos, sampling, streams, stop_tokens, stop_sequences, stop_frame, return_logits,
                      constraints=None, repeat=None):
        """`generate` on the job-control path: the sampler launch (`evo_sample_rows_ctl_f32`) ends a row's job on the device.  The host
        knows the step by which a slot MUST have finished (its limit) and, with a stop rule, reads the [S] lengths every `poll_every`
        steps to learn which slots finished sooner; a finished slot's history rows [:length] are fetched, its store row released, the
        slot re-filled.  Here: the rule is checked and copied into the per-pool state the captured launch reads; _run does the rest."""
        m, tok, S, dev = self.model, self.tok, self.n_slots, self.device
        if int(stop_frame) < 1:
            raise ValueError("stop_frame must be >= 1")
        patterns = stop_patterns(tok, stop_sequences)
        stop_set = None
        if stop_tokens is not None and len(stop_tokens):
            stop_set = allowed_mask(tok, stop_tokens)
            if self.allow_mask is not None and bool((stop_set & ~self.allow_mask).any()):
                raise ValueError("stop_tokens: a stop token outside allowed_tokens could never be drawn")
        for p in patterns:
            if self.allow_mask is not None and not all(bool(self.allow_mask[t]) for t in p):
                raise ValueError("stop_sequences: a pattern with a token outside allowed_tokens could never be drawn")
        if not prompts:
            return [], [], []
        if not hasattr(m.ops, "sample_rows_ctl"):
            raise RuntimeError("stop rules and per-prompt lengths need a compute backend with sample_rows_ctl; this model's backend has none")
        per_prompt, distinct = self._constraints_of(constraints, len(prompts)) if constraints is not None else (None, [])
        if distinct and not hasattr(m.ops, "sample_rows_dfa"):
            raise RuntimeError("constraints need a compute backend with sample_rows_dfa; this model's backend has none")
        rc = None
        if repeat is not None:                                       #  every refusal before any device work
            if not isinstance(repeat, RepeatControl):
                raise ValueError("repeat: one RepeatControl for the call")
            rc = repeat.resolve(tok, self.allow_mask)
            if not Backend.adopt(m.ops).supports("repeat"):
                raise RuntimeError('repeat needs a compute backend with the "repeat" kernels (' + ", ".join(Backend.OPTIONAL["repeat"])
                                   + "); this model's backend has none")
        encoded = [prepare_batch([p], tok, prepend_bos=prepend_bos, device=str(dev))[0] for p in prompts]
        has_stop = stop_set is not None or bool(patterns) or bool(distinct)      # (a job may end by completing its constraint: the host polls)
        has_stop = has_stop or (rc is not None and rc.end_num > 0)   # (... or by the repeat rule)
        was_device = self.device_sampler
        self.device_sampler = True                                   # (as with allowed_tokens alone: no seed means seed 0)
        try:
            # jobs of unequal length: a store row per live slot, or one per prompt (a layout without a store sizes itself from the limits)
            self.kv.size([e.shape[1] for e in encoded], limits, n_spp, rows=min(S, len(prompts)))
            if self.s_limit is None:
                self._allocate_sampler_state()
            self._allocate_history_ctl(max(limits), return_logits)
            # everything the captured launch reads by address is per-pool state; the rule is copied INTO it.  What travels by value --
            # the patterns, the frame, whether there is a stop mask at all -- is the key the captured step is kept under
            if stop_set is not None:
                self.s_stop_mask.copy_(m.ops.pack_allow_mask(stop_set, dev))
            dfa, bases = self._upload_constraints(per_prompt, distinct) if distinct else (None, None)
            self._ctl = {"stop_mask": None if stop_set is None else self.s_stop_mask,
                         "stop_seq": m.ops.pack_stop_sequences(patterns) if patterns else None, "stop_frame": int(stop_frame), "dfa": dfa,
                         "repeat": None}
            if rc is not None:                                       # alphabet, k, end_min_tokens and "armed" travel by value: part of the key
                self._allocate_repeat(rc)
                self._ctl["repeat"] = {"alphabet": torch.tensor(rc.ids, dtype=torch.int32), "k": rc.k, "end_min_tokens": rc.end_min_tokens,
                                       "armed": rc.end_num > 0}
            # (the alphabet travels by value; the table is read by address and its size is an argument)
            key = ("ctl", tuple(map(tuple, patterns)), int(stop_frame), stop_set is not None) \
                + ((distinct[0].alphabet, dfa["next"].data_ptr(), int(dfa["next"].shape[0])) if distinct else ()) \
                + (("repeat", rc.k, rc.ids, rc.end_min_tokens, rc.end_num > 0) if rc is not None else ())
            if key != self._graph_key:
                self._graph, self._graph_key = None, key
            for name in ("stop_ends", "length_ends", "polls", "idle_slot_steps") + (("constraint_ends",) if distinct else ()) \
                    + (("repeat_ends",) if rc is not None else ()):
                self.stats.setdefault(name, 0)
            return self._run("ctl", prompts, encoded, limits, n_spp, sampling, streams, has_stop, return_logits, bases, rc)
        finally:
            self.device_sampler = was_device

    def _run(self, mode, prompts, encoded, limits, n_spp, sampling, streams, has_stop=False, return_logits=True, dfa_bases=None, rc=None):
        """The one scheduling loop of generate(): admit (FIFO; fill = prefill lookup, install, sampler settings, first token), step, look
        (who finished), fetch (results out, slots released).  `mode` supplies what a step is, the first token and what fetch copies out:
        "host" (the reference's sampler on logits read back every step), "rows" (`sample_rows`, every job `limits[0]` tokens long) or
        "ctl" (`sample_rows_ctl` / `_dfa`, with the repeat launch in front when `rc`); only "ctl" under a stop rule reads the device to
        learn who finished."""
        m, tok, S, dev, kv = self.model, self.tok, self.n_slots, self.device, self.kv
        host, ctl = mode == "host", mode == "ctl"
        rep_init: Dict[int, tuple] = {}                              # repeat control: a prompt's starting state, shared by its copies
        if rc is not None:                                           # one RepeatControl per call: every slot's levels and fraction
            self.s_rep_levels.copy_(rc.levels.to(dev)[None, :].expand(S, 8))
            self.s_rep_end.fill_(rc.end_num)
        L = max(limits)
        # job = (output index, prompt index); the copies of one prompt are adjacent so that they share a prefill
        jobs = deque((pi * n_spp + c, pi) for pi in range(len(prompts)) for c in range(n_spp))
        n_jobs = len(jobs)
        out_ids = torch.full((n_jobs, L), -1 if ctl else 0, dtype=torch.long)
        out_logprobs = torch.zeros(n_jobs, L, dtype=torch.float32) if ctl else None
        out_logits = torch.zeros(n_jobs, L, m.vocab_size, dtype=torch.float32) if return_logits else None
        out_len, out_fin = [0] * n_jobs, [0] * n_jobs
        out_rep: List[Tuple[int, int]] = [(0, 0)] * n_jobs
        slot_job: List[Optional[int]] = [None] * S
        slot_n = [0] * S                                             # tokens the slot's job has if it is still running
        slot_limit = [0] * S
        cached_prefill: Dict[int, tuple] = {}
        need_of = [kv.need(e.shape[1] + n) for e, n in zip(encoded, limits)]

        # ---- what a mode supplies: the first token (from the prefill's last logits), a step, what fetch copies out
        def first_host(slot: int, j: int, pi: int, last_logits) -> None:
            first = sample(last_logits[None], top_k=self.top_k, top_p=self.top_p, temperature=self.temperature)
            out_ids[j, 0] = int(first[0])
            out_logits[j, 0] = last_logits.cpu()
            self.ids[slot, 0] = first[0]

        def first_rows(slot: int, j: int, pi: int, last_logits) -> None:
            self.s_active[slot] = True
            self._sample_rows(last_logits[None], slice(slot, slot + 1), None)

        def first_ctl(slot: int, j: int, pi: int, last_logits) -> None:
            self.s_limit[slot] = limits[pi]
            self.s_length[slot] = -1
            self.s_finish[slot] = 0
            if dfa_bases is not None:                                # the job starts in state 0 of its prompt's automaton
                self.s_dfa_base[slot] = dfa_bases[pi]
                self.s_dfa_state[slot] = 0
            self.s_active[slot] = True
            if rc is not None:                                       # the prompt's k-mers; nothing generated yet; the first row through the launch
                if pi not in rep_init:
                    rep_init.clear()
                    rep_init[pi] = self._repeat_init(encoded[pi][0], rc)
                self.s_rep_counts[slot], self.s_rep_ctx[slot] = rep_init[pi]
                self.s_rep_stat[slot] = 0
                self._repeat_rows(last_logits[None], slice(slot, slot + 1), fed=False)
                last_logits = self.s_rep_logits[slot]
            self._sample_rows_ctl(last_logits[None], slice(slot, slot + 1))      # the first token; with limit 1 (or a stop) also the last

        def step_host(active: List[int]) -> None:
            logits = self._step()                                     # [S, V]
            nxt = sample(logits, top_k=self.top_k, top_p=self.top_p, temperature=self.temperature)
            lg_cpu, nxt_cpu = logits.cpu(), nxt.cpu()
            self.ids[:, 0] = nxt
            kv.advance()
            for s in active:
                out_ids[slot_job[s], slot_n[s]] = nxt_cpu[s]
                out_logits[slot_job[s], slot_n[s]] = lg_cpu[s]

        def collect_rows(slots: List[int], idx, lengths) -> None:
            """Their history rows leave the device (the only read-back of the device sampler)."""
            self.s_active[idx] = False
            ids_cpu, lg_cpu = self.hist_ids[idx, :L].cpu(), self.hist_logits[idx, :L].cpu()
            for r, s in enumerate(slots):
                out_ids[slot_job[s]], out_logits[slot_job[s]] = ids_cpu[r], lg_cpu[r]

        def collect_ctl(slots: List[int], idx, lengths) -> None:
            """Rows [:length] of their histories leave the device.  `lengths` None: every one of them ran to its limit (no stop rule:
            nothing to ask the device)."""
            if lengths is None:
                lengths, fins = [slot_limit[s] for s in slots], [FINISH_LENGTH] * len(slots)
            else:
                fins = self.s_finish[idx].cpu().tolist()
                if FINISH_DEAD_END in fins:                          # (validate() rules it out for every reachable state)
                    raise RuntimeError("decode pool: a constrained job reached a state that permits no token")
            n_max = max(lengths)
            ids_cpu, lp_cpu = self.hist_ids[idx, :n_max].cpu(), self.hist_logprob[idx, :n_max].cpu()
            lg_cpu = self.hist_logits[idx, :n_max].cpu() if return_logits else None
            rep_cpu = self.s_rep_stat[idx].cpu().tolist() if rc is not None else None
            for r, s in enumerate(slots):
                j, n = slot_job[s], int(lengths[r])
                if rc is not None:
                    out_rep[j] = (int(rep_cpu[r][0]), int(rep_cpu[r][1]))
                out_ids[j, :n], out_logprobs[j, :n] = ids_cpu[r, :n], lp_cpu[r, :n]
                if return_logits:
                    out_logits[j, :n] = lg_cpu[r, :n]
                out_len[j], out_fin[j] = n, int(fins[r])
                self.stats[{FINISH_LENGTH: "length_ends", FINISH_CONSTRAINT: "constraint_ends", FINISH_REPEAT: "repeat_ends"}.get(fins[r], "stop_ends")] += 1
                self.stats["idle_slot_steps"] += slot_n[s] - n
                self.stats["tokens"] -= slot_n[s] - n                # (steps a finished slot sat through generate nothing)

        first, step, collect = {"host": (first_host, step_host, None), "rows": (first_rows, lambda active: self._step_sampled(), collect_rows),
                                "ctl": (first_ctl, lambda active: self._step_sampled(), collect_ctl)}[mode]

        def fill(slot: int) -> None:
            j, pi = jobs.popleft()
            if pi not in cached_prefill:
                self._prefill_for(pi, jobs, slot_job, encoded, cached_prefill)
            last_logits, tmp, row = cached_prefill[pi]
            P = encoded[pi].shape[1]
            # (row 0 of a B = 1 prefill, nothing to reserve: the call as it always was)
            kv.install(slot, pi, tmp, P, **{k: v for k, v in (("row", row), ("need", need_of[pi])) if v})
            if not host:
                # the job's settings and its own random stream (its output index); the first token is draw 0 of that stream,
                # taken by the same kernel from the prefill's last logits
                cfg = (sampling[pi] if sampling is not None else None) or {}
                self.s_top_k[slot] = int(cfg.get("top_k", self.top_k))
                self.s_top_p[slot] = float(cfg.get("top_p", self.top_p))
                self.s_temperature[slot] = float(cfg.get("temperature", self.temperature))
                self.s_stream[slot] = j if streams is None else int(streams[j])
                self.s_count[slot] = 0
            first(slot, j, pi, last_logits)
            self.pos[slot] = P                                        # the sampled token sits at position P
            slot_job[slot], slot_n[slot], slot_limit[slot] = j, 1, limits[pi]

        def fetch(slots: List[int], lengths: Optional[List[int]]) -> None:
            """Finished slots: the layout takes back what they held, their results leave the device, the slots go idle."""
            kv.release(slots)
            if collect is not None:
                collect(slots, torch.tensor(slots, dtype=torch.int64, device=dev), lengths)
            for s in slots:
                slot_job[s] = None

        done, since_poll = 0, 0
        while done < n_jobs:
            filled, waiting = False, 0
            for s in range(S):
                if slot_job[s] is None and jobs:
                    if waiting or not kv.can_admit(need_of[jobs[0][1]]):     # the head of the queue waits for what it reserves (FIFO)
                        waiting += 1
                        continue
                    fill(s)
                    filled = True
                    if slot_limit[s] == 1 and not has_stop:
                        fetch([s], None)
                        done += 1
            active = [s for s in range(S) if slot_job[s] is not None]
            if not active:
                continue
            # Under a stop rule a job may end on its first token, which fill() drew: after a round of fills the host looks before it
            # steps (the fetch that emptied those slots has synchronised anyway).  due: slots whose job has ended by now for sure.
            look = has_stop and filled
            due = [s for s in active if slot_n[s] >= slot_limit[s]]
            if not look and not due:
                if self.share_prompt_kv:
                    self._count_prefix_streams()
                if waiting:
                    self.stats["kv_page_waits"] += waiting
                step(active)
                since_poll += 1
                for s in active:
                    slot_n[s] += 1
                self.stats["tokens"] += len(active)
                due = [s for s in active if slot_n[s] >= slot_limit[s]]
            if not has_stop:
                finished, lengths = due, None                         # lengths are the limits: the host knows without reading
            elif look or due or since_poll >= self.poll_every or not jobs or waiting:
                # the one read: [S] lengths, -1 while a job runs.  With nothing left to admit the host looks after every step: no step
                # may run with every row already ended.  While the head of the queue waits for pages (kv_paged) it looks after every step too:
                # a job that ended sooner frees the pages the head needs
                polled = self.s_length.cpu().tolist()
                self.stats["polls"] += 1
                since_poll = 0
                finished = [s for s in active if polled[s] >= 0]
                lengths = [polled[s] for s in finished]
                if any(s not in finished for s in due):
                    raise RuntimeError("decode pool: a slot ran past its limit without ending on the device")
            else:
                finished = []
            if finished:
                fetch(finished, lengths)
                done += len(finished)

        owner = [pi for pi in range(len(prompts)) for _ in range(n_spp)]
        self.last_ids, self.last_logits = out_ids, out_logits        # (kept for inspection / tests)
        for name in ("last_lengths", "last_finish", "last_logprobs", "last_repeats"):    # (an earlier job-control run's: they would describe that run)
            self.__dict__.pop(name, None)
        if not ctl:
            lp = logits_to_logprobs(out_logits, out_ids).float().numpy()   # the reference's shifted pairing
            return list(tok.detokenize_batch(out_ids)), [float(np.mean(lp[j])) for j in range(n_jobs)], owner
        self.last_logprobs, self.last_lengths, self.last_finish = out_logprobs, list(out_len), [FINISH_NAMES_REPEAT[f] for f in out_fin]
        if rc is not None:
            self.last_repeats = list(out_rep)
        seqs, scores = [], []
        for j in range(n_jobs):
            n = out_len[j] - (1 if out_fin[j] == FINISH_STOP_TOKEN else 0)      # a stop token is trimmed, a stop sequence stays
            seqs.append(tok.detokenize(out_ids[j, :n].tolist()))
            scores.append(float(np.mean(out_logprobs[j, :out_len[j]].numpy().astype(np.float64))))
        return seqs, scores, owner


    # ------------------------------------------------------------------ beam search
    def _allocate_beam(self, W: int, n_tokens: int, has_stop: bool) -> dict:
        """Per-pool state of a beam search: the per-slot vectors the selection launch reads and writes, the back-pointer history, and the
        table of every per-slot record the reparenting copy moves.  Bound to the caches it registers: new caches, a new width or a longer
        history make new state and drop the captured beam step."""
        m, S, dev, ops = self.model, self.n_slots, self.device, self.model.ops
        key = (W, has_stop)
        b = self._beam
        if b is not None and b["ipd"] is self.ipd and b["key"] == key and b["hist_parent"].shape[1] >= n_tokens:
            return b
        G = S // W
        hy, mha = self.ipd["hyena"], self.ipd["mha"]
        if getattr(ops, "beam_cum_dtype", torch.float32) == torch.float64:       # an fp64 backend: the search keeps the modal state in its precision too
            for i in m.hyena_layer_idxs:
                hy.state_dict[i] = hy.state_dict[i].to(torch.complex128)
        fixed =[hy.fir_state_dict[i] for i in m.hyena_layer_idxs] + [hy.state_dict[i] for i in m.hyena_layer_idxs]
        table = ops.gather_table(fixed, [mha.key_value_memory_dict[i] for i in m.attn_layer_idxs])
        L = n_tokens
        b = {"key": key, "ipd": self.ipd, "W": W, "G": G, "table": table,
             "cum": torch.full((S,), float("-inf"), dtype=getattr(ops, "beam_cum_dtype", torch.float32), device=dev),
             "ended": torch.zeros(S, dtype=torch.uint8, device=dev), "length": torch.zeros(S, dtype=torch.int64, device=dev),
             "parent": torch.arange(S, dtype=torch.int64, device=dev), "active": torch.zeros(G, dtype=torch.uint8, device=dev),
             "admit": torch.zeros(G, dtype=torch.uint8, device=dev), "step": torch.zeros(G, dtype=torch.int64, device=dev),
             "hist_parent": torch.zeros(S, L, dtype=torch.int32, device=dev), "hist_ids": torch.zeros(S, L, dtype=torch.int64, device=dev),
             "hist_cum": torch.zeros(S, L, dtype=getattr(ops, "beam_cum_dtype", torch.float32), device=dev),
             "first": torch.zeros(S, m.vocab_size, dtype=getattr(ops, "beam_cum_dtype", torch.float32), device=dev),
             "allow": None if self.allow_mask is None else ops.pack_allow_mask(self.allow_mask, dev),
             "stop": torch.zeros(64, dtype=torch.uint8, device=dev) if has_stop else None}
        self._beam, self._beam_graph = b, None
        self.stats["beam_scratch_bytes"] = int(getattr(table, "scratch_bytes", 0))
        return b

    def _beam_select(self, logits: torch.Tensor, group_active: torch.Tensor) -> None:
        b = self._beam
        self.model.ops.beam_select(logits, b["cum"], b["ended"], b["length"], self.ids, b["parent"], b["W"], group_active=group_active,
                                   allow=b["allow"], stop_mask=b["stop"], hist_parent=b["hist_parent"], hist_ids=b["hist_ids"],
                                   hist_cum=b["hist_cum"], step=b["step"])

    def _step_beam_eager(self) -> None:
        """Forward, selection, the reparenting copy (out, then back), advance: every slot's records follow the hypothesis it now holds."""
        b = self._beam
        self._beam_select(self._step_eager(), b["active"])
        self.model.ops.gather_rows(b["table"], b["parent"], self.store.own_pos)
        self.kv.advance()

    def _step_beam(self) -> None:
        self.stats["steps"] += 1
        self.stats["beam_steps"] += 1
        _, self._beam_graph = self._captured(self._beam_graph, self._step_beam_eager)

    def beam_search(self, prompts: Sequence[str], n_tokens: int, beam_width: int = 4, stop_tokens=None, prepend_bos: bool = False,
                    return_steps: bool = False, **refused) -> List["BeamResult"]:
        """The `beam_width` most likely continuations of every prompt, by total log-probability: one `BeamResult` per
        prompt, its hypotheses in rank order.  A prompt owns a group of `beam_width` consecutive slots; n_slots // beam_width prompts are
        searched together, a finished group is fetched and re-filled while the others go on.  Needs `share_prompt_kv=True`; uses the
        pool's `allowed_tokens`; `stop_tokens` end a hypothesis (it keeps its score and competes on) and are trimmed from its string; one
        outside `allowed_tokens` can never be chosen and is harmless.  A
        group is over after `n_tokens` steps, or sooner when every beam has ended (the host looks every `poll_every` steps).  No length
        penalty, no temperature, no top-k / top-p.  `return_steps=True`: every result also carries the recorded per-step
        (parent, token, cum) of its group."""
        for name in ("constraints", "stop_sequences", "seed"):
            if refused.pop(name, None) is not None:
                raise ValueError(f"beam_search: {name} is not supported (a search is deterministic, and ends hypotheses on stop TOKENS only)")
        if refused:
            raise TypeError(f"beam_search: unexpected arguments {sorted(refused)}")
        if self.batch_invariant:
            raise ValueError("beam_search does not combine with batch_invariant=True (a beam group's attention splits by group)")
        m, tok, S, dev = self.model, self.tok, self.n_slots, self.device
        W = int(beam_width)
        if not 1 <= W <= 8 or W > S:
            raise ValueError(f"beam_width must be 1 ... 8 and at most n_slots = {S}, got {beam_width}")
        if not self.share_prompt_kv:
            raise ValueError("beam_search needs a pool built with share_prompt_kv=True (a beam group reads one stored copy of its prompt)")
        if self.kv_dtype != "bf16" or self.kv_paged:                 # (such a pool cannot be built with share_prompt_kv; kept for the day it can)
            raise ValueError('beam_search does not combine with kv_dtype="fp8" or kv_paged=True')
        n_tokens = int(n_tokens)
        prompts, limits, _ = self._check_job(prompts, n_tokens, prepend_bos=prepend_bos, beam=True)
        stop_set = None
        if stop_tokens is not None and len(stop_tokens):
            stop_set = allowed_mask(tok, stop_tokens)
        if not Backend.adopt(m.ops).supports("beam"):
            raise RuntimeError('beam_search needs a compute backend with the "beam" kernels (beam_select, gather_rows); this model\'s backend '
                               "has none")
        if hasattr(m, "eval"):
            m.eval()
        encoded = [prepare_batch([p], tok, prepend_bos=prepend_bos, device=str(dev))[0] for p in prompts]
        self.kv.size([e.shape[1] for e in encoded], limits, W, rows=min(S // W, len(prompts)))     # one store row per group
        b = self._allocate_beam(W, n_tokens, stop_set is not None)
        if stop_set is not None:
            b["stop"].copy_(m.ops.pack_allow_mask(stop_set, dev))
        for name in ("beam_groups", "beam_steps", "beam_rows_moved", "polls"):
            self.stats.setdefault(name, 0)
        return self._run_beam(prompts, encoded, n_tokens, stop_set, return_steps)

    def _run_beam(self, prompts, encoded, n_tokens, stop_set, return_steps):
        m, tok, S, dev, b = self.model, self.tok, self.n_slots, self.device, self._beam
        W, G = b["W"], b["G"]
        jobs = deque((pi, pi) for pi in range(len(prompts)))         # (job, prompt) as _prefill_for reads them: one job per prompt
        results: List[Optional[BeamResult]] = [None] * len(prompts)
        group_job: List[Optional[int]] = [None] * G
        group_n = [0] * G                                            # selections the group has been through (the admission's is the first)
        cached_prefill: Dict[int, tuple] = {}
        neg_inf = float("-inf")

        def fill(g: int) -> None:
            _, pi = jobs.popleft()
            if pi not in cached_prefill:
                self._prefill_for(pi, jobs, group_job, encoded, cached_prefill, logits_dtype=b["first"].dtype)
            last_logits, tmp, row = cached_prefill[pi]
            P = encoded[pi].shape[1]
            rows = slice(g * W, g * W + W)
            for s in range(g * W, g * W + W):                        # one store row; every slot of the group holds the prompt's states
                self.kv.install(s, pi, tmp, P, **({"row": row} if row else {}))
            b["cum"][rows] = neg_inf
            b["cum"][g * W] = 0.0
            b["ended"][rows] = 0
            b["length"][rows] = 0
            b["step"][g] = 0
            self.ids[rows, 0] = encoded[pi][0, -1]
            # the group's first selection is the same launch on the prefill's last logits: one live beam seeds W (nothing to move yet:
            # the group's slots hold the same records)
            b["first"][rows] = last_logits.to(b["first"].dtype)
            b["admit"].zero_()
            b["admit"][g] = 1
            self._beam_select(b["first"], b["admit"])
            self.pos[rows] = P
            b["active"][g] = 1
            group_job[g], group_n[g] = pi, 1
            self.stats["beam_groups"] += 1

        def fetch(groups: List[int]) -> None:
            """Finished groups: their back-pointers and final state leave the device; the hypotheses are rebuilt on the host."""
            slots = [s for g in groups for s in range(g * W, g * W + W)]
            idx = torch.tensor(slots, dtype=torch.int64, device=dev)
            self.kv.release(slots)
            b["active"][torch.tensor(groups, dtype=torch.int64, device=dev)] = 0
            T = max(min(group_n[g], n_tokens) for g in groups)
            hp, hi, hc = b["hist_parent"][idx, :T].cpu(), b["hist_ids"][idx, :T].cpu(), b["hist_cum"][idx, :T].cpu()
            cum, length, ended = b["cum"][idx].cpu(), b["length"][idx].cpu().tolist(), b["ended"][idx].cpu().tolist()
            for k, g in enumerate(groups):
                Tg, lo = min(group_n[g], n_tokens), k * W
                res = BeamResult([], [], [], [])
                for j in range(W):
                    if not bool(cum[lo + j] > neg_inf):
                        continue
                    toks, s = [], g * W + j
                    for col in range(Tg - 1, -1, -1):                # walk the back-pointers
                        toks.append(int(hi[lo + s - g * W, col]))
                        s = int(hp[lo + s - g * W, col])
                    toks = toks[::-1][:length[lo + j]]               # (beyond its length an ended hypothesis only repeats its last token)
                    n_text = len(toks) - (1 if ended[lo + j] and stop_set is not None and toks and bool(stop_set[toks[-1]]) else 0)
                    res.sequences.append(tok.detokenize(toks[:n_text]))
                    res.scores.append(float(cum[lo + j]))
                    res.lengths.append(int(length[lo + j]))
                    res.mean_scores.append(float(cum[lo + j]) / max(int(length[lo + j]), 1))
                own = torch.arange(g * W, g * W + W, dtype=hp.dtype)[:, None]
                self.stats["beam_rows_moved"] += int(((hp[lo:lo + W, 1:Tg] != own) & (hc[lo:lo + W, 1:Tg] > neg_inf)).sum())
                if return_steps:
                    res.steps = (hp[lo:lo + W, :Tg].clone(), hi[lo:lo + W, :Tg].clone(), hc[lo:lo + W, :Tg].clone())
                results[group_job[g]] = res
                group_job[g] = None

        done, since_poll = 0, 0
        while done < len(prompts):
            filled = False
            for g in range(G):
                if group_job[g] is None and jobs:
                    fill(g)
                    filled = True
            active = [g for g in range(G) if group_job[g] is not None]
            due = [g for g in active if group_n[g] >= n_tokens]
            look = stop_set is not None and filled                    # (a hypothesis may end on its first token)
            if not due and not look:
                self._count_prefix_streams()
                self._step_beam()
                since_poll += 1
                for g in active:
                    group_n[g] += 1
                self.stats["tokens"] += len(active) * W
                due = [g for g in active if group_n[g] >= n_tokens]
            finished = due
            if stop_set is not None and (look or due or since_poll >= self.poll_every or not jobs):
                # the one read: is every beam of a group ended or empty?  (with nothing left to admit the host looks after every step)
                over = (b["ended"].bool() | ~(b["cum"] > neg_inf))[:G * W].view(G, W).all(-1).cpu().tolist()
                self.stats["polls"] += 1
                since_poll = 0
                finished = [g for g in active if over[g] or g in due]
            if finished:
                fetch(finished)
                done += len(finished)
        return results


class BeamResult:
    """What `beam_search` returns for one prompt: its non-empty hypotheses in rank order -- `sequences` (a stop token trimmed), `scores`
    (total log-probability), `lengths` (tokens generated, the stop token included), `mean_scores` (score / length, to re-rank with) --
    and, with return_steps=True, `steps` = (parent, token, cum), each [beam_width, steps run]: what every selection gave the group's
    slots (parent: a slot index of the pool)."""

    def __init__(self, sequences, scores, lengths, mean_scores, steps=None):
        self.sequences, self.scores, self.lengths, self.mean_scores, self.steps = sequences, scores, lengths, mean_scores, steps

    def __len__(self):
        return len(self.sequences)

    def __repr__(self):
        return f"BeamResult(sequences={self.sequences!r}, scores={self.scores!r}, lengths={self.lengths!r})"


def beam_search(prompts: Sequence[str], model, tokenizer, n_tokens: int, beam_width: int = 4, n_slots: Optional[int] = None,
                allowed_tokens=None, stop_tokens=None, prefill_batch: int = 1, weight_dtype: str = "bf16", device: Optional[str] = None,
                prepend_bos: bool = False, return_steps: bool = False, poll_every: int = 8) -> List[BeamResult]:
    """The `beam_width` most likely continuations of every prompt (`DecodePool.beam_search` on a pool of its own with
    `share_prompt_kv=True`).  `n_slots` defaults to beam_width * min(len(prompts), 32 // beam_width)."""
    prompts = list(prompts)
    W = int(beam_width)
    if not 1 <= W <= 8:
        raise ValueError(f"beam_width must be 1 ... 8, got {beam_width}")
    if not prompts:
        raise ValueError("beam_search: the prompt list is empty")
    if n_slots is None:
        n_slots = W * min(len(prompts), 32 // W)
    pool = DecodePool(model, tokenizer, n_slots=n_slots, device=device, allowed_tokens=allowed_tokens, share_prompt_kv=True,
                      prefill_batch=prefill_batch, weight_dtype=weight_dtype, poll_every=poll_every)
    return pool.beam_search(prompts, n_tokens, beam_width=W, stop_tokens=stop_tokens, prepend_bos=prepend_bos, return_steps=return_steps)


def sample_many(prompts: Sequence[str], model, tokenizer, n_tokens: int = 1000, temp: float = 0.7, top_k: int = 4,
                top_p: float = 1.0, n_sample_per_prompt: int = 1, n_slots: int = 8, prepend_bos: bool = False,
                device: Optional[str] = None, seed: Optional[int] = None, allowed_tokens=None, share_prompt_kv: bool = False,
                prefill_batch: int = 1, stop_tokens=None, stop_sequences=None, stop_frame: int = 1, return_logits: bool = True,
                poll_every: int = 8, constraints=None, kv_dtype: str = "bf16", weight_dtype: str = "bf16", kv_paged: bool = False,
                kv_page_tokens: int = 256, kv_budget_tokens: Optional[int] = None, batch_invariant: bool = False,
                repeat: Optional[RepeatControl] = None):
    """`semantic_design.run_model` / `sample_model` without the equal-length restriction: (prompts repeated per
    sample, generated sequences, scores).  `seed` makes the run reproducible (for a fixed `n_slots`), `allowed_tokens`
    (e.g. "ACGT") restricts what may be drawn; either moves the sampler onto the device.  `share_prompt_kv`: the
    samples of a prompt read one stored copy of its K/V.  `prefill_batch` > 1: up to that many prompts admitted
    together are prefilled in one forward, right-padded.  `n_tokens` as a sequence (one limit per prompt),
    `stop_tokens`, `stop_sequences` / `stop_frame` and `return_logits=False`: jobs that end on their own (see
    `DecodePool.generate`).  `constraints`: one `TokenConstraint` (evo_amd/constraints.py) for every prompt, or one (or None) per prompt --
    constrained generation on the device.  `kv_dtype="fp8"`: the pool's KV cache in FP8 e4m3fn, about half the bytes
    (not with `share_prompt_kv`).  `kv_paged=True`: the KV cache is a pool of pages of `kv_page_tokens` tokens, a job
    holds what its own prompt and limit need, and `kv_budget_tokens` caps the pool (not with `share_prompt_kv` or
    `kv_dtype="fp8"`).  `batch_invariant=True`: with a `seed`, every job's result is the same bits at any `n_slots` from 1 to 64 (DESIGN.md
    section 25; not with `prefill_batch` > 1, `share_prompt_kv`, `kv_dtype="fp8"` or `weight_dtype="fp8"`).  `repeat`: one
    `RepeatControl` -- a penalty on nucleotides that would complete a k-mer the job has seen, and optionally an early end for jobs that
    turned repetitive."""
    pool = DecodePool(model, tokenizer, n_slots=n_slots, top_k=top_k, top_p=top_p, temperature=temp, device=device, seed=seed,
                      allowed_tokens=allowed_tokens, share_prompt_kv=share_prompt_kv, prefill_batch=prefill_batch, poll_every=poll_every,
                      kv_dtype=kv_dtype, weight_dtype=weight_dtype, kv_paged=kv_paged, kv_page_tokens=kv_page_tokens,
                      kv_budget_tokens=kv_budget_tokens, batch_invariant=batch_invariant)
    ctl = {}
    if stop_tokens is not None or stop_sequences is not None or int(stop_frame) != 1 or not return_logits:
        ctl = dict(stop_tokens=stop_tokens, stop_sequences=stop_sequences, stop_frame=stop_frame, return_logits=return_logits)
    if constraints is not None:
        ctl["constraints"] = constraints
    if repeat is not None:
        ctl["repeat"] = repeat
    seqs, scores, owner = pool.generate(prompts, n_tokens=n_tokens, n_sample_per_prompt=n_sample_per_prompt,
                                        prepend_bos=prepend_bos, **ctl)
    return [prompts[i] for i in owner], seqs, scores

