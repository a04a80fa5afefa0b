"""TEST INFRASTRUCTURE: the launch sequence of the host forward, as data.

`recording(ops)` puts a recording proxy around `ops.lib` for the duration of a block.  For every entry point called it notes the name,
every argument whose declared type in `evo_amd.ops._SIGNATURES` is an integer or a float (taken from the argtypes, never guessed from
the value) and, for every pointer argument, only whether it was null; the call is then forwarded unchanged.  No address goes into the
record, and the stream -- the last argument of every launch (include/evo_mi355x.h, Conventions) -- is left out altogether.

SCENARIOS names the forwards whose traces tests/golden/forward_trace.json pins (tests/test_gpu_forward_trace.py): every route of the
Hyena and attention blocks, every in-process knob, the caches, the pool, variant scoring, embeddings and one sequence-parallel rank.
Each scenario returns the tensors / arrays it computed; their bytes are hashed next to the trace.

`python tests/forward_trace.py [FILE]` writes the golden file (or FILE): every scenario runs twice, and a digest is stored only where both runs agree
(null otherwise: the trace still pins the scenario).  The file is written from the code whose behaviour is to be kept, and a
host-side refactor never regenerates it.
"""
import contextlib
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_trace.json")
DEV = "cuda:0"

_INTS = (ctypes.c_int64, ctypes.c_int, ctypes.c_int32, ctypes.c_uint64)
_FLOATS = (ctypes.c_float, ctypes.c_double)


def describe(name, argtypes, args):
    """One call as a string: the entry point, then one token per argument but the stream -- the integer, the float as the library
    receives it, or `&` / `null` for a pointer."""
    assert len(args) == len(argtypes), (name, len(args), len(argtypes))
    out = [name]
    for t, a in list(zip(argtypes, args))[:-1]:
        if t in _INTS:
            out.append(str(int(a)))
        elif t in _FLOATS:
            out.append(repr(t(a).value))
        else:
            out.append("null" if a is None or (isinstance(a, int) and a == 0) else "&")
    return " ".join(out)


class _RecordingLib:
    def __init__(self, lib, calls, signatures):
        self._lib, self._calls, self._signatures = lib, calls, signatures

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        sig = self._signatures.get(name)
        if sig is None or not sig[0]:
            return fn

        def call(*args):
            self._calls.append(describe(name, sig[0], args))
            return fn(*args)
        return call


@contextlib.contextmanager
def recording(ops):
    """-> the list the calls made through `ops.lib` inside the block are appended to."""
    from evo_amd.ops import _SIGNATURES
    calls, real = [], ops.lib
    ops.lib = _RecordingLib(real, calls, _SIGNATURES)
    try:
        yield calls
    finally:
        ops.lib = real


def digest(results) -> str:
    """SHA-256 over the bytes of every tensor / array of a scenario's result, in order."""
    h = hashlib.sha256()
    for r in results:
        if isinstance(r, torch.Tensor):
            r = r.detach().cpu().contiguous()
            r = r.view(torch.int16) if r.dtype == torch.bfloat16 else r
            r = r.numpy()
        h.update(np.ascontiguousarray(r).tobytes())
    return h.hexdigest()


# ---- the models: the two small configs of tests/test_gpu_model.py, built once, every decode step eager -----------------------------
# (shared by all scenarios: what a forward leaves on a model -- the rotary cache, folded / regrouped weight copies, operand tables -- is made
# by torch alone and changes no launch; a scenario that flips a knob of `ops` puts it back)
_MODELS = {}


def model(which):
    """`SMALL` / `SMALL4` of tests/test_gpu_model.py (seed 0), or `SMALL4-folded`: SMALL4 after prepare().fold_norms_()."""
    if which not in _MODELS:
        import test_gpu_model as G
        m = G.build(getattr(G, which.split("-")[0]))[2]
        m.decode_graph = False
        if which.endswith("-folded"):
            m.prepare().fold_norms_()
        _MODELS[which] = m
    return _MODELS[which]


def ids_of(B, T, seed=1234):
    """[B, T] ids: a BOS token in front of T - 1 nucleotides (tests/test_gpu_model.py acgt)."""
    from test_gpu_model import acgt
    return acgt(B, T - 1, seed).to(DEV)


# ---- scenarios -------------------------------------------------------------------------------------------------------------------
def _stateless(which, B, T, mask=False):
    def run():
        m, ids = model(which), ids_of(B, T)
        pm = None
        if mask:
            pm = torch.ones(B, T, dtype=torch.int64)
            pm[0, T - 37:] = 0
            pm[1, T - 5:] = 0
        return [m(ids, padding_mask=pm)[0]]
    return run


def _knob_off(knob):
    def run():
        ops = model("SMALL4").ops
        assert getattr(ops, knob) is True
        setattr(ops, knob, False)
        try:
            return _stateless("SMALL4", 2, 1025)()
        finally:
            setattr(ops, knob, True)
    return run


def _cached(which, P, resumed=40, steps=3, B=2):
    """Prefill of P tokens, a resumed prefill of `resumed` more (halo and carry-in), then single-token steps."""
    def run():
        m = model(which)
        ids = ids_of(B, P + resumed + steps)
        c = m.initialize_inference_params()
        c["mha"].max_batch_size = c["hyena"].max_batch_size = B
        out, t = [], 0
        for n in [P] + ([resumed] if resumed else []) + [1] * steps:
            c["mha"].seqlen_offset = c["hyena"].seqlen_offset = t
            out.append(m(ids[:, t:t + n], c)[0])
            t += n
        return out
    return run


def _one_token_prefill():
    """A fresh cache whose prefill is ONE token (T < K1: the FIR history is zero-padded), then a single-token step."""
    return _cached("SMALL", 1, resumed=0, steps=1)()


def _ragged(lens=(130, 200, 77)):
    m = model("SMALL")
    ids = ids_of(len(lens), max(lens))
    logits, ipd = m.prefill_ragged(ids, list(lens))
    out = [logits]
    pos = torch.tensor(lens, dtype=torch.int64, device=DEV)
    tok = logits.argmax(-1, keepdim=True)
    for _ in range(2):                                       # per-row-position decode steps
        ipd["mha"].pos_tensor = pos
        try:
            lg = m(tok, ipd)[0]
        finally:
            ipd["mha"].pos_tensor = None
        out.append(lg)
        tok = lg[:, 0].float().argmax(-1, keepdim=True)
        pos = pos + 1
    return out


def _variants():
    from evo_amd.scoring import score_variants
    from evo_amd.tokenizer import CharLevelTokenizer
    rng = np.random.default_rng(77)
    ref = "".join(rng.choice(list("ACGT"), size=700))
    variants = []
    for p in (100, 600, 650):                                # one in front of the checkpoint at 512, two behind it
        variants.append(ref[:p] + "ACGT"[("ACGT".index(ref[p]) + 1) % 4] + ref[p + 1:])
    vs = score_variants(ref, variants, model("SMALL"), CharLevelTokenizer(512), checkpoint_every=512, device=DEV)
    assert vs.stats["cached"] and vs.stats["checkpoints"] == [512]
    return [vs.score, vs.delta]


def _pool(gen=None, seed=5, which="SMALL", **kw):
    """A 4-slot pool on SMALL (or `which`), every step eager: PROMPTS[0] and PROMPTS[2], 2 copies, 4 tokens -- the smallest job that re-fills a slot.
    `gen`: arguments of generate() (they replace the defaults); `kw`: arguments of the pool."""
    def run():
        from evo_amd.pool import DecodePool
        from evo_amd.tokenizer import CharLevelTokenizer
        from test_gpu_pool import PROMPTS
        pool = DecodePool(model(which), CharLevelTokenizer(512), n_slots=4, device=DEV, use_graph=False, seed=seed, **kw)
        pool.generate([PROMPTS[0], PROMPTS[2]], **dict(dict(n_tokens=4, n_sample_per_prompt=2), **(gen or {})))
        out = [pool.last_ids] + ([] if pool.last_logits is None else [pool.last_logits])
        if hasattr(pool, "last_lengths"):                        # a job-control run
            out += [pool.last_logprobs, np.array(pool.last_lengths, dtype=np.int64)]
        return out
    return run


def _job_control():
    """Jobs that end on their own: one limit per prompt, the three stop codons in frame, ACGT only, no logits kept, a look every 2 steps."""
    return dict(gen=dict(n_tokens=[4, 2], stop_sequences=["TAA", "TAG", "TGA"], stop_frame=3, return_logits=False),
                allowed_tokens="ACGT", poll_every=2)


def _pool_constrained():
    from evo_amd.constraints import iupac_template
    return _pool(gen=dict(constraints=[iupac_template("ANR"), None]), allowed_tokens="ACGT")()


def _pool_repeat():
    from evo_amd.sh.sample import RepeatControl
    return _pool(gen=dict(repeat=RepeatControl(k=3, penalty=0.5, end_fraction=0.25, end_min_tokens=2)), allowed_tokens="ACGT")()


def _pool_w8():
    model("SMALL")._w8 = None                                # the FP8 copies are quantised inside the scenario, whichever ran before it
    return _pool(weight_dtype="fp8")()


def _beam():
    from evo_amd.pool import DecodePool
    from evo_amd.tokenizer import CharLevelTokenizer
    from test_gpu_pool import PROMPTS
    pool = DecodePool(model("SMALL"), CharLevelTokenizer(512), n_slots=4, device=DEV, use_graph=False, share_prompt_kv=True,
                      allowed_tokens="ACGT")
    res = pool.beam_search([PROMPTS[0], PROMPTS[2]], 4, beam_width=2, stop_tokens="T", return_steps=True)
    return [t for r in res for t in r.steps] + [np.array([r.scores for r in res], dtype=np.float64)]


def _embeddings():
    out = model("SMALL").embeddings(ids_of(2, 300), layers=[1, "final"], pooling="mean")
    return [out[1], out["final"]]


def _sp(which, B, T, rank, attn_mode):
    def run():
        from evo_amd.sp import SequenceParallelScorer, StubComm
        sp = SequenceParallelScorer(model(which), rank, 2, comm=StubComm(2))
        sp.attn_mode = attn_mode
        return [sp.score_logprobs(ids_of(B, T))]
    return run


KNOBS = ("fuse_norm", "hyena_tail_split", "mlp_gate_fused", "hyena_mfma", "hyena_ct_flag", "attn_prescale", "attn_w64", "all_gemm_mfma")

SCENARIOS = {
    # stateless scoring on SMALL4: each shape the smallest that reaches its branch
    "score 2x1025 tail form r=1, tail split, folded": _stateless("SMALL4", 2, 1025),
    "score 1x2050 tail form r=2, no split": _stateless("SMALL4", 1, 2050),
    "score 4x1280 plain form, stream rows, folded": _stateless("SMALL4", 4, 1280),
    "score 3x700 padded rows, folded MLP, unfolded pre-norm": _stateless("SMALL4", 3, 700),
    "score 2x300 below the 1024-row floor": _stateless("SMALL4", 2, 300),
    "score 2x20 modal kernels": _stateless("SMALL4", 2, 20),
    "score 2x300 padding mask": _stateless("SMALL4", 2, 300, mask=True),
    **{f"score 2x1025 {k}=False": _knob_off(k) for k in KNOBS},
    "one weight set: score 2x1025": _stateless("SMALL4-folded", 2, 1025),
    "one weight set: prefill 513 + 3 steps": _cached("SMALL4-folded", 513, resumed=0),
    "cache P=513 + 40 + 3 steps": _cached("SMALL", 513),
    "cache P=513 + 200 (channel-major resume) + 1 step": _cached("SMALL", 513, resumed=200, steps=1),
    "cache P=600 + 40 + 3 steps": _cached("SMALL", 600),
    "cache P=20 + 40 + 3 steps": _cached("SMALL", 20),
    "cache P=1 (T < K1) + 1 step": _one_token_prefill,
    "prefill_ragged (130, 200, 77) + 2 per-row steps": _ragged,
    "prefill_ragged (20, 9) modal form + 2 per-row steps": lambda: _ragged((20, 9)),
    "score_variants 700 nt, 3 substitutions": _variants,
    "pool 2x2, 4 slots, shared prompt K/V, prefill_batch=2": _pool(share_prompt_kv=True, prefill_batch=2),
    "pool 2x2, 4 slots, defaults": _pool(),
    # the pool's scheduler, one scenario per path through it (pinned before evo_amd/pool.py was restructured)
    "pool 2x2, 4 slots, host sampler, greedy": _pool(seed=None, top_k=1),
    "pool 2x2, 4 slots, job control: limits [4, 2], stop codons in frame 3, ACGT, no logits, poll_every=2": _pool(**_job_control()),
    "pool 2x2, 4 slots, job control on shared prompt K/V (store rows per prompt)": _pool(share_prompt_kv=True, **_job_control()),
    "pool 2x2, 4 slots, one IUPAC template and one free prompt": _pool_constrained,
    "pool 2x2, 4 slots, repeat control k=3 with end_fraction": _pool_repeat,
    "pool 2x2, 4 slots, kv_dtype=fp8": _pool(kv_dtype="fp8"),
    "pool 2x2, 4 slots, weight_dtype=fp8": _pool_w8,
    "pool 2x2, 4 slots, kv_paged, 64-token pages, budget 7 pages (the head waits)": _pool(kv_paged=True, kv_page_tokens=64, kv_budget_tokens=448),
    "pool 2x2, 4 slots, batch_invariant (SMALL4: the row-invariant gate needs I % 32 == 0)": _pool(which="SMALL4", batch_invariant=True),
    "pool 2x2, 4 slots, n_tokens=1": _pool(gen=dict(n_tokens=1)),
    "pool 2x2, 4 slots, n_tokens=1, host sampler": _pool(seed=None, top_k=1, gen=dict(n_tokens=1)),
    "pool beam_search width 2, 4 slots, stop token T": _beam,
    "embeddings [1, final] mean 2x300": _embeddings,
    **{f"sp rank {r} of 2, 2x2050, attn {mode}": _sp("SMALL4", 2, 2050, r, mode) for r in (0, 1) for mode in ("auto", "allgather")},
    **{f"sp rank {r} of 2, 2x60 modal stages": _sp("SMALL", 2, 60, r, "auto") for r in (0, 1)},
}


def run_scenario(name):
    """-> (trace: list of call strings, digest of the result)."""
    from evo_amd.ops import default_ops
    torch.manual_seed(0)
    with recording(default_ops()) as calls:
        with torch.no_grad():
            results = SCENARIOS[name]()
        torch.cuda.synchronize()
    return calls, digest(results)


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def main():
    golden, unstable = {}, []
    for name in SCENARIOS:
        t1, d1 = run_scenario(name)
        t2, d2 = run_scenario(name)
        assert t1 == t2, f"{name}: two runs made different launches"
        if d1 != d2:
            unstable.append(name)
        golden[name] = {"digest": d1 if d1 == d2 else None, "trace": t1}
        print(f"{name}: {len(t1)} calls, digest {'stable' if d1 == d2 else 'NOT reproducible'}", flush=True)
    if len(unstable) > 2:
        raise SystemExit(f"{len(unstable)} scenarios are not bit-reproducible -- not writing a golden that pins little: {unstable}")
    out = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    with open(out, "w") as f:
        json.dump(golden, f, indent=0, separators=(",", ":"))
        f.write("\n")
    print(f"wrote {out} ({os.path.getsize(out)} bytes); not reproducible: {unstable}")


if __name__ == "__main__":
    here = os.path.dirname(os.path.abspath(__file__))
    for p in (os.path.dirname(here), here):
        if p not in sys.path:
            sys.path.insert(0, p)
    main()
