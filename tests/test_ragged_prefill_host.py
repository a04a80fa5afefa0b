"""CPU: ragged batched prefill (StripedHyena.prefill_ragged, DecodePool prefill_batch) on the fp64 oracle backend.

The backend is tests/oracle_ops.OracleOps (through test_fanout_host.FanoutOracleOps, for the shared-K/V pool) plus `hyena_state_at` built
from its own `hyena_end_state` row by row -- the definition of what the kernel of csrc/hyena_ragged.hip computes -- and the operator
evaluated by its recurrence instead of an FFT (RaggedOracleOps.hyena_prefill says why).

  * prefill_ragged on prompts of 1, 2, 3, 37 and 130 tokens against five B = 1 cached prefills: last logits, every FIR state, every modal
    state and KV[b, :L_b], each within 1e-9 x max|x|.  In fp64 only the summation order of batched matmuls can differ; the bound sits seven
    orders above fp64 epsilon and far below any real defect (a pad reaching a valid position, a state taken at T instead of L_b);
  * another token in the pad columns leaves every returned tensor torch.equal;
  * DecodePool(prefill_batch=4), greedy, against prefill_batch=1: tokens, owners, strings, logits, the forwards the admission rule predicts;
  * prefill_batch=1 leaves `stats` without the new keys; Generator refuses a ragged cache; the forms that cannot be ragged raise ValueError."""
import pytest
import torch

from evo_amd.generation import Generator
from evo_amd.pool import DecodePool
from test_fanout_host import SMALL, TOK, FanoutOracleOps
from test_gpu_pool import PROMPTS

LENS = [1, 2, 3, 37, 130]
N_TOK = 6
TOL = 1e-9


class RaggedOracleOps(FanoutOracleOps):
    """+ the per-row end state: row b's state and FIR history are those of z[b, :lens[b]] alone."""

    def __init__(self, act=torch.float64):
        super().__init__(act)
        self.state_at_calls = 0

    def hyena_prefill(self, z, fir_w, fir_b, poles, residues, dskip, n_heads, z_halo=None, s0=None, want_state=False, seg_len=None,
                      mask=None):
        """The operator by its recurrence, step by step in fp64.  OracleOps evaluates the long convolution with an FFT over the whole row:
        exact to ~1e-15, but every output then carries rounding noise of every input of the row, pads included -- the bitwise pad test
        below needs an operator that is causal in its BITS, as the engine's kernels are.  Same function, same precision."""
        if z_halo is not None or s0 is not None or mask is not None:
            return super().hyena_prefill(z, fir_w, fir_b, poles, residues, dskip, n_heads, z_halo, s0, want_state, seg_len, mask)
        B, T, D3 = z.shape
        D, hd = D3 // 3, D3 // 3 // n_heads
        zp = torch.cat([z.new_zeros(B, 2, D3), z.double()], dim=1)
        w = fir_w.double()
        zc = fir_b.double() + sum(w[:, k] * zp[:, k:k + T] for k in range(3))
        z4 = zc.view(B, T, n_heads, 3, hd)
        x2, x1, v = (z4[:, :, :, g].reshape(B, T, D) for g in range(3))
        x = x1 * v
        p = torch.view_as_complex(poles.double().contiguous())
        r = torch.view_as_complex(residues.double().contiguous())
        S = torch.zeros(B, D, p.shape[1], dtype=torch.complex128)
        ys = []
        for t in range(T):
            S = p * S + x[:, t, :, None]
            ys.append((r * S).real.sum(-1))
        out = (torch.stack(ys, dim=1) + x * dskip.double()) * x2
        return self._o(out), (S if want_state else None)

    def hyena_state_at(self, z, lens, fir_w, fir_b, poles, n_heads):
        self.state_at_calls += 1
        states, firs = [], []
        for b, n in enumerate(int(v) for v in lens):
            zb = z[b:b + 1, :n]
            states.append(self.hyena_end_state(zb, fir_w, fir_b, poles, n_heads))
            tail = zb[:, -2:]
            if n < 2:
                tail = torch.cat([zb.new_zeros(1, 2 - n, z.shape[-1]), tail], dim=1)
            firs.append(tail.transpose(1, 2))
        return torch.cat(states, 0), torch.cat(firs, 0).contiguous()


@pytest.fixture(scope="module")
def small():
    from oracle.stripedhyena_ref import RefConfig, make_synthetic_state_dict
    from evo_amd.sh.model import StripedHyena
    sd = make_synthetic_state_dict(RefConfig.from_dict(SMALL), seed=3)
    m = StripedHyena(dict(SMALL), ops=RaggedOracleOps(torch.float64))
    m.load_state_dict({k: (v.double() if v.dtype == torch.bfloat16 else v) for k, v in sd.items()})
    return m


def _ids(filler):
    g = torch.Generator().manual_seed(5)
    T = max(LENS)
    ids = torch.randint(0, 256, (len(LENS), T), generator=g)
    for b, n in enumerate(LENS):
        ids[b, n:] = filler if filler is not None else ids[b, n - 1]
    return ids


def _flat(logits, ipd, m):
    """name -> tensor, KV cut to every row's own length."""
    out = {"logits": logits}
    for i in m.hyena_layer_idxs:
        out[f"fir{i}"] = ipd["hyena"].fir_state_dict[i]
        out[f"state{i}"] = torch.view_as_real(ipd["hyena"].state_dict[i])
    for i in m.attn_layer_idxs:
        for b, n in enumerate(LENS):
            out[f"kv{i}.{b}"] = ipd["mha"].key_value_memory_dict[i][b, :n]
    return out


@pytest.fixture(scope="module")
def ragged(small):
    small.ops.state_at_calls = 0
    logits, ipd = small.prefill_ragged(_ids(None), LENS)
    assert small.ops.state_at_calls == len(small.hyena_layer_idxs)
    return logits, ipd


def test_ragged_prefill_equals_every_prompt_alone(small, ragged):
    logits, ipd = ragged
    T_pad = -(-max(LENS) // 64) * 64
    assert logits.shape == (len(LENS), small.vocab_size) and logits.dtype == torch.float32
    assert ipd["mha"].lengths.tolist() == LENS and ipd["hyena"].lengths.tolist() == LENS
    for i in small.attn_layer_idxs:
        assert tuple(ipd["mha"].key_value_memory_dict[i].shape[:2]) == (len(LENS), T_pad)
    got = _flat(logits, ipd, small)
    ids = _ids(None)
    for b, n in enumerate(LENS):
        tmp = small.initialize_inference_params()
        tmp["mha"].max_seqlen = n
        lg, tmp = small(ids[b:b + 1, :n], inference_params_dict=tmp)
        want = {"logits": lg[0, -1].float()}
        for i in small.hyena_layer_idxs:
            want[f"fir{i}"] = tmp["hyena"].fir_state_dict[i][0]
            want[f"state{i}"] = torch.view_as_real(tmp["hyena"].state_dict[i])[0]
        for i in small.attn_layer_idxs:
            want[f"kv{i}.{b}"] = tmp["mha"].key_value_memory_dict[i][0, :n]
        for name, w in want.items():
            g = got[name] if name.startswith("kv") else got[name][b]
            assert g.shape == w.shape, (name, b, g.shape, w.shape)
            err, top = float((g.double() - w.double()).abs().max()), float(w.double().abs().max())
            print(f"row {b} (L = {n}) {name}: max err {err:.3e} of max {top:.3e}")
            assert err <= TOL * top, (name, b, err, top)


def test_pad_tokens_reach_nothing(small, ragged):
    a = _flat(*ragged, small)
    for filler in (7, 300):
        b = _flat(*small.prefill_ragged(_ids(filler), LENS), small)
        assert a.keys() == b.keys()
        for name in a:
            assert torch.equal(a[name], b[name]), (filler, name)
    # and the width it is rounded to does not matter either
    c = _flat(*small.prefill_ragged(_ids(7), LENS, pad_to=8), small)
    for name in a:
        assert torch.equal(a[name], c[name]), ("pad_to", name)


def test_the_forms_that_cannot_be_ragged_are_refused(small, ragged):
    ids = _ids(None)
    with pytest.raises(ValueError):
        small.prefill_ragged(ids, LENS, padding_mask=torch.ones_like(ids))
    with pytest.raises(ValueError):
        small.prefill_ragged(ids, LENS, inference_params_dict=ragged[1])
    with pytest.raises(ValueError):
        small.prefill_ragged(ids, [0] + LENS[1:])
    with pytest.raises(ValueError):
        small.prefill_ragged(ids, LENS[:-1] + [max(LENS) + 1])
    with pytest.raises(ValueError):
        small.prefill_ragged(ids, LENS[:-1])
    with pytest.raises(ValueError):                                       # a second multi-token forward on the ragged cache: resumed prefill
        small(ids, inference_params_dict=ragged[1])
    from evo_amd.sh.cache import SharedPrefix
    ipd = small.initialize_inference_params()
    ipd["mha"].lengths = ipd["hyena"].lengths = torch.tensor(LENS)
    ipd["mha"].shared_prefix = SharedPrefix()
    with pytest.raises(ValueError):
        small(ids, inference_params_dict=ipd)


def test_generator_refuses_a_ragged_cache(small, ragged):
    gen = Generator(small, TOK, top_k=1)
    with pytest.raises(ValueError, match="ragged"):
        gen.generate("cpu", input_ids=_ids(None), num_tokens=2, inference_params_dict=ragged[1], print_generation=False)


# ------------------------------------------------------------------------------------------------ the pool
def _pool(m, n_slots, share, prefill_batch):
    kw = {} if prefill_batch is None else {"prefill_batch": prefill_batch}
    return DecodePool(m, TOK, n_slots=n_slots, top_k=1, top_p=1.0, temperature=0.0, device="cpu", share_prompt_kv=share, **kw)


def predicted_forwards(lengths, n_samples, n_slots, batch, cap=32768, pad=64):
    """The admission rule, restated: jobs have one length, so the slots go idle together and take the jobs in waves of n_slots; a prompt
    without a prefill takes along the distinct prompts among the jobs the slots still idle will take -- at most `batch`, and stopping
    before (prompts) x (longest, rounded up to `pad`) exceeds `cap`; the prefill before it is dropped."""
    jobs = [pi for pi in range(len(lengths)) for _ in range(n_samples)]
    forwards, have = 0, set()
    for k in range(0, len(jobs), n_slots):
        wave = jobs[k:k + n_slots]
        for q, pi in enumerate(wave):
            if pi in have:
                continue
            group, t_max = [], 0
            for p in wave[q:]:
                if p in group:
                    continue
                t = max(t_max, -(-lengths[p] // pad) * pad)
                if len(group) == batch or (group and (len(group) + 1) * t > cap):
                    break
                group.append(p)
                t_max = t
            have = set(group)
            forwards += 1
    return forwards


@pytest.fixture(scope="module")
def one_by_one(small):
    out = {}
    for n_slots in (4, 8):
        pool = _pool(small, n_slots, False, None)
        seqs, scores, owner = pool.generate(PROMPTS, n_tokens=N_TOK, n_sample_per_prompt=3)
        assert pool.stats["prefills"] == len(PROMPTS)
        assert "prefill_prompts" not in pool.stats and "prefill_pad_tokens" not in pool.stats
        out[n_slots] = (pool.last_ids.clone(), pool.last_logits.clone(), seqs, owner)
    return out


@pytest.mark.parametrize("share", [False, True])
@pytest.mark.parametrize("n_slots", [4, 8])
def test_batched_prefill_pool_equals_the_pool_one_by_one(small, one_by_one, n_slots, share):
    want_ids, want_logits, want_seqs, want_owner = one_by_one[n_slots]
    pool = _pool(small, n_slots, share, 4)
    seqs, scores, owner = pool.generate(PROMPTS, n_tokens=N_TOK, n_sample_per_prompt=3)
    assert owner == want_owner and seqs == want_seqs
    assert torch.equal(pool.last_ids, want_ids)
    err, top = float((pool.last_logits.double() - want_logits.double()).abs().max()), float(want_logits.abs().max())
    print(f"{n_slots} slots, share {share}: logits max err {err:.3e} of max {top:.3e}")
    assert err <= TOL * top
    lengths = [len(p) for p in PROMPTS]
    want = predicted_forwards(lengths, 3, n_slots, 4)
    assert want == {4: 4, 8: 2}[n_slots] and want < len(PROMPTS)
    assert pool.stats["prefills"] == want
    assert pool.stats["prefill_prompts"] == len(PROMPTS)
    assert pool.stats["prefill_pad_tokens"] > 0
    if share:
        assert pool.stats["prompt_kv_installs"] == len(PROMPTS) and pool.store_refs == [0] * len(pool.store_refs)


def test_the_token_cap_and_the_default(small, one_by_one):
    want_ids, want_logits, _, _ = one_by_one[8]
    lengths = [len(p) for p in PROMPTS]
    # a cap of 256 padded positions: the first wave's prompts (80, 8, 145 tokens) fit as 2 x 128 but not as 3 x 192
    pool = DecodePool(small, TOK, n_slots=8, top_k=1, top_p=1.0, temperature=0.0, device="cpu", prefill_batch=4, prefill_max_tokens=256)
    pool.generate(PROMPTS, n_tokens=N_TOK, n_sample_per_prompt=3)
    want = predicted_forwards(lengths, 3, 8, 4, cap=256)
    assert pool.stats["prefills"] == want and 2 < want < len(PROMPTS)
    assert pool.stats["prefill_prompts"] == len(PROMPTS) and torch.equal(pool.last_ids, want_ids)
    # a cap below any prompt: every prompt alone, through the B = 1 prefill -- bit for bit the pool without the option
    pool = DecodePool(small, TOK, n_slots=8, top_k=1, top_p=1.0, temperature=0.0, device="cpu", prefill_batch=4, prefill_max_tokens=1)
    pool.generate(PROMPTS, n_tokens=N_TOK, n_sample_per_prompt=3)
    assert pool.stats["prefills"] == len(PROMPTS) and pool.stats["prefill_pad_tokens"] == 0
    assert torch.equal(pool.last_ids, want_ids) and torch.equal(pool.last_logits, want_logits)
    with pytest.raises(ValueError):
        DecodePool(small, TOK, n_slots=2, device="cpu", prefill_batch=0)
