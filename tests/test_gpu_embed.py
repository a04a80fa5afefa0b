"""GPU (-m gpu): sequence embeddings -- the pooling kernel (csrc/pool.hip) against fp64 torch, StripedHyena.embeddings' early exit
against the block_taps streams of a full forward (bit for bit), pooled embeddings against the fp64 / bf16-faithful oracle's block
streams, ragged batches against sequences embedded alone, the identity-unembed recipe, and scripts/embed.py end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import stripedhyena_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = dict(vocab_size=512, hidden_size=256, num_layers=4, attn_layer_idxs=[2], num_attention_heads=2)


def rel_l2(a, ref):
    a, ref = a.double().cpu(), ref.double().cpu()
    return ((a - ref).norm() / ref.norm()).item()


def build(cfgd, seed=0):
    from evo_amd.sh.model import StripedHyena
    cfg = R.RefConfig.from_dict(cfgd)
    sd = R.make_synthetic_state_dict(cfg, seed)
    m = StripedHyena(dict(cfgd))
    m.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    m.to_bfloat16_except_poles_residues()
    return cfg, sd, m.to(DEV)


def acgt(B, L, seed=1234):
    rows = [np.random.default_rng(seed + b).choice(np.frombuffer(b"ACGT", dtype=np.uint8), size=L) for b in range(B)]
    return torch.cat([torch.zeros(B, 1, dtype=torch.long), torch.from_numpy(np.stack(rows).astype(np.int64))], dim=1)


def pool_ref64(x, ranges, scale, eps, mode, chunk=8192):
    """fp64 torch: mean / last of f(x) over each range, f = RMSNorm (eps outside the root) with `scale`, identity without."""
    D = x.shape[1]
    outs = []
    for a, n in ranges:
        if mode == "last":
            a, n = a + n - 1, 1
        acc = torch.zeros(D, dtype=torch.float64, device=x.device)
        for c in range(a, a + n, chunk):
            r = x[c:min(a + n, c + chunk)].double()
            if scale is not None:
                r = r / (r.norm(dim=1, keepdim=True) * D ** -0.5 + eps)
            acc += r.sum(0)
        acc /= n
        outs.append(acc * scale.double() if scale is not None else acc)
    return torch.stack(outs)


@pytest.mark.parametrize("D", [256, 4096])
@pytest.mark.parametrize("mode", ["mean", "last"])
@pytest.mark.parametrize("norm", [False, True])
def test_pool_kernel_vs_fp64_ragged(D, mode, norm):
    from evo_amd.ops import default_ops
    ops = default_ops()
    g = torch.Generator(device=DEV).manual_seed(D + 7 * norm)
    lens = [1, 17, 3000, 640, 1234]                                 # B = 5, ragged, 1 ... 3,000 rows
    firsts = np.concatenate([[3], 3 + np.cumsum(lens)[:-1] + 5]).tolist()    # gaps between ranges: rows that must not be pooled
    M = firsts[-1] + lens[-1] + 2
    x = (torch.randn(M, D, device=DEV, generator=g) * 1.5 + 0.5).to(torch.bfloat16)
    x[0:3] = 1e4                                                    # (outside every range)
    scale = (torch.rand(D, device=DEV, generator=g) + 0.5).to(torch.bfloat16) if norm else None
    ranges = list(zip(firsts, lens))
    got = ops.pool_rows(x, ranges, scale=scale, eps=1e-6, mode=mode)
    want = pool_ref64(x, ranges, scale, 1e-6, mode)
    assert got.shape == (5, D) and got.dtype == torch.float32
    for b in range(5):
        assert rel_l2(got[b], want[b]) <= 1e-5, (b, rel_l2(got[b], want[b]))
    again = ops.pool_rows(x, ranges, scale=scale, eps=1e-6, mode=mode)
    assert torch.equal(got, again)                                  # no atomics: bit-identical run to run
    # a row pitch above D (a column slice of a wider matrix)
    wide = torch.zeros(M, D + 64, dtype=torch.bfloat16, device=DEV)
    wide[:, :D] = x
    assert torch.equal(ops.pool_rows(wide[:, :D], ranges, scale=scale, eps=1e-6, mode=mode), got)


def test_pool_kernel_one_long_row_at_bench_size():
    """1 x 131,073 x 4096 (the 131k bench shape's stream, 1.07 GB): mean with the fused norm, and without."""
    from evo_amd.ops import default_ops
    ops = default_ops()
    g = torch.Generator(device=DEV).manual_seed(5)
    T, D = 131073, 4096
    x = torch.empty(T, D, dtype=torch.bfloat16, device=DEV)
    for c in range(0, T, 16384):
        x[c:c + 16384] = (torch.randn(min(16384, T - c), D, device=DEV, generator=g) + 0.25).to(torch.bfloat16)
    scale = (torch.rand(D, device=DEV, generator=g) + 0.5).to(torch.bfloat16)
    ranges = [(1, T - 1)]
    for sc in (scale, None):
        got = ops.pool_rows(x, ranges, scale=sc, eps=1e-6, mode="mean")
        err = rel_l2(got, pool_ref64(x, ranges, sc, 1e-6, "mean"))
        print(f"[pool 1 x {T} x {D} norm={sc is not None}] rel-L2 vs fp64 {err:.2e}")
        assert err <= 1e-5
        assert torch.equal(got, ops.pool_rows(x, ranges, scale=sc, eps=1e-6, mode="mean"))
    del x
    torch.cuda.empty_cache()


def _taps(m, ids, idxs):
    """block_taps of a full hidden_states: the stream entering block i for i in idxs (index num_layers = the final stream)."""
    m.block_taps, m.block_tap_idxs = [], set(idxs)
    try:
        hid = m.hidden_states(ids)
        return hid, dict(zip(sorted(idxs), m.block_taps))
    finally:
        m.block_taps, m.block_tap_idxs = None, None


def test_early_exit_is_exact_small():
    cfg, sd, m = build(SMALL)
    ids = acgt(2, 300).to(DEV)
    B, T = ids.shape
    hid, taps = _taps(m, ids, {1, 3, 4})
    calls = []
    orig = (m._hyena_block, m._attn_block)
    m._hyena_block = lambda i, *a, **k: (calls.append(i), orig[0](i, *a, **k))[1]
    m._attn_block = lambda i, *a, **k: (calls.append(i), orig[1](i, *a, **k))[1]
    try:
        for k in (0, 2, 3):                                          # first block, the attention block, the last block
            calls.clear()
            got = m.embeddings(ids, [k], pooling="none")[k]
            assert calls == list(range(k + 1))                       # stops after block k
            assert torch.equal(got.view(B * T, -1), taps[k + 1]), k
        calls.clear()
        fin = m.embeddings(ids, ["final"], pooling="none")["final"]
        assert calls == [0, 1, 2, 3] and torch.equal(fin.view(B * T, -1), hid)
    finally:
        del m._hyena_block, m._attn_block


def test_early_exit_is_exact_7b(full):
    m = full["m8"]
    ids = acgt(1, 512).to(DEV)
    B, T = ids.shape
    with torch.inference_mode():
        hid, taps = _taps(m, ids, {1, 9, 32})
        got = m.embeddings(ids, [0, 8, 31, "final"], pooling="none")
        for k in (0, 8, 31):
            assert torch.equal(got[k].view(B * T, -1), taps[k + 1]), k
        assert torch.equal(got["final"].view(B * T, -1), hid)
        assert torch.equal(m.embeddings(ids, [8], pooling="none")[8].view(B * T, -1), taps[9])
        # pooled: the kernel on the same streams
        pooled = m.embeddings(ids, [8, "final"], pooling="mean")
        assert rel_l2(pooled[8][0], taps[9][1:].double().mean(0)) < 1e-5
        x = taps[32][1:].double()
        want = (m.norm.scale.double() * x / (x.norm(dim=1, keepdim=True) * 4096 ** -0.5 + m.eps)).mean(0)
        assert rel_l2(pooled["final"][0], want) < 1e-5


def _oracle_streams(o, ids):
    """Per block, the residual stream leaving it, and the final-norm output, of the oracle (its own block loop)."""
    x = o.w["embedding_layer.weight"][ids.long()]
    out = {}
    for i in range(o.cfg.num_layers):
        x = o.attn_block(x, i, None) if i in o.cfg.attn_layer_idxs else o.hyena_block(x, i, None)
        out[i] = x
    out["final"] = o.rmsnorm(x, o.w["norm.scale"])
    return out


def test_pooled_embeddings_vs_oracle_small():
    cfg, sd, m = build(SMALL)
    ids = acgt(2, 400)
    lengths = [400, 250]                                             # row 1: its last 150 positions are treated as pads
    layers = [0, 1, 2, 3, "final"]
    got = {p: m.embeddings(ids.to(DEV), layers, pooling=p, lengths=lengths) for p in ("mean", "last")}
    o64 = _oracle_streams(R.RefStripedHyena(cfg, sd, "fp64"), ids)
    o16 = _oracle_streams(R.RefStripedHyena(cfg, sd, "bf16"), ids)

    def pool(s, p):
        return torch.stack([s[b, 1:1 + n].double().mean(0) if p == "mean" else s[b, n].double() for b, n in enumerate(lengths)])

    for p in ("mean", "last"):
        for l in layers:
            ref = pool(o64[l], p)
            floor = rel_l2(pool(o16[l], p), ref)
            err = rel_l2(got[p][l], ref)
            print(f"[embeddings SMALL {p} layer {l}] rel-L2 hip {err:.2e}, bf16-oracle floor {floor:.2e}")
            assert err < max(1.5 * floor, 4e-3), (p, l, err, floor)


def test_ragged_batch_matches_sequences_alone():
    import evo_amd
    from evo_amd.tokenizer import CharLevelTokenizer
    cfg, sd, m = build(SMALL)
    tok = CharLevelTokenizer(512)
    rng = np.random.default_rng(3)
    seqs = ["".join(rng.choice(list("ACGT"), size=n)) for n in (700, 33, 1500, 1)]
    for pooling in ("mean", "last", "none"):
        batch = evo_amd.embed_sequences(seqs, m, tok, layers=[1, "final"], pooling=pooling, device=DEV)
        for i, s in enumerate(seqs):
            alone = evo_amd.embed_sequences([s], m, tok, layers=[1, "final"], pooling=pooling, device=DEV)
            for l in (1, "final"):
                a, b = np.asarray(batch[l][i], np.float64), np.asarray(alone[l][0], np.float64)
                assert a.shape == b.shape == ((len(s), 256) if pooling == "none" else (256,))
                err = np.linalg.norm(a - b) / np.linalg.norm(b)
                assert err < 1e-2, (pooling, i, l, err)


def test_identity_unembed_recipe_and_unembed_method():
    import torch.nn as nn
    from evo_amd.scoring import _fused_tail_ok
    cfg, sd, m = build(SMALL)
    ids = acgt(2, 200).to(DEV)
    B, T = ids.shape
    logits, _ = m(ids)
    hid = m.hidden_states(ids)
    assert torch.equal(m.unembed.unembed(hid.view(B, T, -1)), logits)      # the engine's unembed() = the forward's logits
    assert _fused_tail_ok(m, ids)

    class Identity(nn.Module):
        def unembed(self, u):
            return u

    own = m.unembed
    m.unembed = Identity()
    try:
        emb, _ = m(ids)
        assert torch.equal(emb, hid.view(B, T, -1))
        assert not _fused_tail_ok(m, ids)
        cache = m.initialize_inference_params()
        assert not m._graph_eligible(cache)
    finally:
        m.unembed = own
    assert torch.equal(m(ids)[0], logits)


def test_embed_cli_matches_in_process(full, tmp_path):
    """scripts/embed.py as a subprocess (evo-1-8k-base, the synthetic weights of the session's 7B fixture) against embed_sequences
    on the fixture's model, same batches."""
    import evo_amd
    from evo_amd.fasta import length_buckets
    from evo_amd.tokenizer import CharLevelTokenizer
    rng = np.random.default_rng(11)
    seqs = ["".join(rng.choice(list("ACGT"), size=n)) for n in (300, 120, 257)]
    names = ["a", "b", "c"]
    fa = tmp_path / "in.fa"
    fa.write_text("".join(f">{n} test\n{s[:60]}\n{s[60:]}\n" for n, s in zip(names, seqs)))
    npz = tmp_path / "out.npz"
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "embed.py"), "--input-fasta", str(fa), "--output-npz", str(npz),
                        "--model-name", "evo-1-8k-base", "--weights", "synthetic", "--device", DEV, "--batch-size", "2",
                        "--layers", "16,final", "--pooling", "mean"], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    z = np.load(npz)
    assert list(z["names"]) == names and z["layer_16"].shape == (3, 4096) and z["final"].shape == (3, 4096)
    tok = CharLevelTokenizer(512)
    want = {16: np.zeros((3, 4096)), "final": np.zeros((3, 4096))}
    for idxs in length_buckets(seqs, 2):
        got = evo_amd.embed_sequences([seqs[i] for i in idxs], full["m8"], tok, layers=[16, "final"], device=DEV)
        for l in want:
            want[l][idxs] = got[l]
    for key, l in (("layer_16", 16), ("final", "final")):
        err = np.linalg.norm(z[key] - want[l]) / np.linalg.norm(want[l])
        print(f"[scripts/embed.py] {key}: rel-L2 vs in-process {err:.2e}")
        assert err < 1e-5
