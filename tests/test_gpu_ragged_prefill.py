"""GPU (-m gpu): ragged batched prefill on the HIP kernels (StripedHyena.prefill_ragged, DecodePool prefill_batch).
SMALL model, prompts of 5, 64, 65, 300 and 513 tokens in one right-padded batch of 5 x 576.

  * two different pad fillers give torch.equal logits, FIR histories, modal states and KV[b, :L_b]: same shapes, same routing, and no pad
    reaches a valid position or a returned state -- bit for bit;
  * accuracy is NOT bitwise against the B = 1 prefill (the row count changes which rows take which dense-layer kernel): the yardstick is
    the fp64 oracle's cached forward of each prompt.  rel-L2 of the last logits and of the modal states, ragged path <= 1.5 x the same
    quantity of five B = 1 prefills on the engine (the same arithmetic in another tiling; the margin covers the noise of a five-row sample);
  * a pooled run with prefill_batch=4 (greedy, 8 slots, 6 tokens): every emitted step's logits against the fp64 oracle's forward of
    prompt + emitted tokens, rel-L2 <= 1.5 x what the prefill_batch=1 pool gives against its own oracle forwards; stats as the
    admission rule predicts;
  * a seeded run with prefill_batch=4, repeated, gives identical strings.
Measured (MI355X): see tests/PARITY_ragged_prefill.md."""
import numpy as np
import pytest
import torch

from oracle import stripedhyena_ref as R
from test_gpu_model import DEV, SMALL, build, rel_l2
from test_ragged_prefill_host import predicted_forwards

pytestmark = pytest.mark.gpu
LENS = [5, 64, 65, 300, 513]
N_TOK = 6


def _prompts():
    rng = np.random.default_rng(2024)
    return ["".join(rng.choice(list("ACGT"), size=n)) for n in LENS]


@pytest.fixture(scope="module")
def world():
    cfg, sd, m = build(SMALL)
    return cfg, sd, m, R.RefStripedHyena(cfg, sd, "fp64")


def _ids(filler):
    T = max(LENS)
    ids = torch.full((len(LENS), T), filler, dtype=torch.long)
    for b, p in enumerate(_prompts()):
        ids[b, :len(p)] = torch.tensor(list(p.encode()), dtype=torch.long)
    return ids


def _flat(logits, ipd, m):
    out = {"logits": logits}
    for i in m.hyena_layer_idxs:
        out[f"fir{i}"] = ipd["hyena"].fir_state_dict[i]
        out[f"state{i}"] = torch.view_as_real(ipd["hyena"].state_dict[i])
    for i in m.attn_layer_idxs:
        for b, n in enumerate(LENS):
            out[f"kv{i}.{b}"] = ipd["mha"].key_value_memory_dict[i][b, :n]
    return out


@pytest.fixture(scope="module")
def ragged(world):
    _, _, m, _ = world
    with torch.inference_mode():
        return m.prefill_ragged(_ids(ord("A")).to(DEV), LENS)


def test_pad_filler_changes_no_bit(world, ragged):
    _, _, m, _ = world
    logits, ipd = ragged
    assert logits.shape == (len(LENS), m.vocab_size) and logits.dtype == torch.float32 and ipd["mha"].lengths.tolist() == LENS
    for i in m.attn_layer_idxs:
        assert tuple(ipd["mha"].key_value_memory_dict[i].shape[:2]) == (len(LENS), 576)
    a = _flat(logits, ipd, m)
    assert all(bool(torch.isfinite(t.float()).all()) for t in a.values())
    with torch.inference_mode():
        b = _flat(*m.prefill_ragged(_ids(ord("T")).to(DEV), LENS), m)
    for name in a:
        assert torch.equal(a[name], b[name]), name


def _count_calls(ops, name, calls):
    fn = getattr(ops, name)

    def spy(*a, **kw):
        calls[name] = calls.get(name, 0) + 1
        return fn(*a, **kw)
    setattr(ops, name, spy)
    return lambda: delattr(ops, name)                                    # (the instance attribute goes, the class's method is back)


@pytest.mark.parametrize("routing", ["channel-major", "modal"])
def test_both_routings_reach_the_kernel_and_stay_causal(world, ragged, routing):
    """The single-pass operator's branch hands z^T to hyena_state_at_zt as it is; the modal branch (layers the table guard refuses, shapes
    the z^T layout refuses -- forced here with hyena_mfma = False) goes through hyena_state_at.  Either way: one call per Hyena layer,
    and another pad filler changes no bit."""
    _, _, m, _ = world
    ops, calls = m.ops, {}
    undo = [_count_calls(ops, "hyena_state_at_zt", calls), _count_calls(ops, "hyena_state_at", calls)]
    was = ops.hyena_mfma
    ops.hyena_mfma = routing == "channel-major"
    try:
        with torch.inference_mode():
            a = _flat(*m.prefill_ragged(_ids(ord("C")).to(DEV), LENS), m)
            n_layers = len(m.hyena_layer_idxs)
            assert calls == ({"hyena_state_at_zt": n_layers} if routing == "channel-major" else {"hyena_state_at_zt": n_layers, "hyena_state_at": n_layers})
            b = _flat(*m.prefill_ragged(_ids(ord("G")).to(DEV), LENS), m)
    finally:
        ops.hyena_mfma = was
        for u in undo:
            u()
    for name in a:
        assert torch.equal(a[name], b[name]), name
    if routing == "channel-major":                                       # (the fixture ran this routing: the same bits again)
        want = _flat(*ragged, m)
        assert all(torch.equal(a[name], want[name]) for name in a)
    else:                                                                # the FIR history is z itself, and z does not depend on the routing's operator in layer 0
        i0 = m.hyena_layer_idxs[0]
        assert rel_l2(a[f"state{i0}"], _flat(*ragged, m)[f"state{i0}"]) < 1e-2


def test_accuracy_is_that_of_five_prefills_alone(world, ragged):
    _, _, m, oracle = world
    ids = _ids(ord("A"))
    ref_lg, ref_st, own_lg, own_st = [], {i: [] for i in m.hyena_layer_idxs}, [], {i: [] for i in m.hyena_layer_idxs}
    for b, n in enumerate(LENS):
        lg, c = oracle(ids[b:b + 1, :n], oracle.initialize_inference_params())
        ref_lg.append(lg[0, -1])
        tmp = m.initialize_inference_params()
        tmp["mha"].max_seqlen = n
        with torch.inference_mode():
            lg1, tmp = m(ids[b:b + 1, :n].to(DEV), inference_params_dict=tmp)
        own_lg.append(lg1[0, -1].float().cpu())
        for i in m.hyena_layer_idxs:
            ref_st[i].append(torch.view_as_real(c["hyena"].state_dict[i][0].resolve_conj()).reshape(-1))
            own_st[i].append(torch.view_as_real(tmp["hyena"].state_dict[i][0]).reshape(-1).cpu())
    logits, ipd = ragged
    e_rag, e_own = rel_l2(logits, torch.stack(ref_lg)), rel_l2(torch.stack(own_lg), torch.stack(ref_lg))
    cat = lambda d: torch.cat([torch.cat(d[i]) for i in m.hyena_layer_idxs])
    rag_st = {i: [torch.view_as_real(ipd["hyena"].state_dict[i][b]).reshape(-1).cpu() for b in range(len(LENS))] for i in m.hyena_layer_idxs}
    s_rag, s_own = rel_l2(cat(rag_st), cat(ref_st)), rel_l2(cat(own_st), cat(ref_st))
    for i in m.hyena_layer_idxs:
        print(f"layer {i} modal states vs fp64: ragged {rel_l2(torch.cat(rag_st[i]), torch.cat(ref_st[i])):.3e}, alone "
              f"{rel_l2(torch.cat(own_st[i]), torch.cat(ref_st[i])):.3e}")
    print(f"last logits vs fp64 oracle: ragged {e_rag:.3e}, five B = 1 prefills {e_own:.3e}; modal states: ragged {s_rag:.3e}, alone {s_own:.3e}")
    assert e_rag <= 1.5 * e_own, (e_rag, e_own)
    assert s_rag <= 1.5 * s_own, (s_rag, s_own)


def _pool_error(world, prefill_batch):
    from evo_amd.pool import DecodePool
    from evo_amd.scoring import prepare_batch
    from evo_amd.tokenizer import CharLevelTokenizer
    _, _, m, oracle = world
    tok = CharLevelTokenizer(512)
    prompts = _prompts()
    pool = DecodePool(m, tok, n_slots=8, top_k=1, top_p=1.0, temperature=0.0, device=DEV, prefill_batch=prefill_batch)
    seqs, scores, owner = pool.generate(prompts, n_tokens=N_TOK, n_sample_per_prompt=2)
    got, want = [], []
    for j, pi in enumerate(owner):
        ids = prepare_batch([prompts[pi]], tok, prepend_bos=False, device="cpu")[0]
        P = ids.shape[1]
        full = torch.cat([ids, pool.last_ids[j:j + 1]], dim=1)
        want.append(oracle(full)[0][0][P - 1:P - 1 + N_TOK])
        got.append(pool.last_logits[j])
    return pool, seqs, owner, rel_l2(torch.stack(got), torch.stack(want))


def test_pool_with_batched_prefill_against_the_oracle(world):
    p1, _, owner1, e1 = _pool_error(world, 1)
    p4, _, owner4, e4 = _pool_error(world, 4)
    print(f"pool logits vs fp64 oracle forwards: prefill_batch=4 {e4:.3e}, prefill_batch=1 {e1:.3e}")
    assert owner1 == owner4 and e4 <= 1.5 * e1, (e4, e1)
    want = predicted_forwards(LENS, 2, 8, 4)
    assert want == 2 and p4.stats["prefills"] == want and p4.stats["prefill_prompts"] == len(LENS)
    assert p4.stats["prefill_pad_tokens"] == 4 * 320 - sum(LENS[:4])
    assert p1.stats["prefills"] == len(LENS) and "prefill_prompts" not in p1.stats


def test_seeded_pool_with_batched_prefill_repeats(world):
    from evo_amd.pool import DecodePool
    from evo_amd.tokenizer import CharLevelTokenizer
    _, _, m, _ = world
    runs = []
    for _ in range(2):
        pool = DecodePool(m, CharLevelTokenizer(512), n_slots=8, top_k=4, top_p=1.0, temperature=0.7, device=DEV, seed=5, prefill_batch=4)
        runs.append(pool.generate(_prompts(), n_tokens=N_TOK, n_sample_per_prompt=2)[0])
    assert runs[0] == runs[1] and len(set(runs[0])) > 1
