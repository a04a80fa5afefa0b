"""CPU: an `ops` object that is NOT a `Backend` still drives the host forward (evo_amd.backend.Backend.adopt).  Before the contract was
written down, `StripedHyena(config, ops=anything)` took any duck-typed object -- the oracle backends of this suite were plain classes
whose rope_ / attention* knew nothing of q_scale / prescaled -- and such stand-ins outside the repository keep working: what they lack
reads as the contract's default (every routing flag off: the modal routes), and the neutral q_scale / prescaled are not passed on."""
import torch

from evo_amd.backend import Backend
from golden_common import TINY
from oracle import stripedhyena_ref as R
from oracle_ops import OracleOps


def _plain(cls):
    """`cls` without the Backend base: its own methods on a plain class, with the rotary / attention signatures of before the contract."""
    body = {k: v for k, v in vars(cls).items() if not k.startswith("__")}
    body["__init__"] = cls.__init__
    body["rope_"] = lambda self, qkv, cos, sin: cls.rope_(self, qkv, cos, sin)
    body["attention"] = lambda self, q, k, v, q_pos0: cls.attention(self, q, k, v, q_pos0)
    body["attention_decode"] = lambda self, q, k, v, pos=None, n_splits=None: cls.attention_decode(self, q, k, v, pos, n_splits)
    return type("Duck" + cls.__name__, (), body)


def _model(ops):
    from evo_amd.sh.model import StripedHyena
    sd = R.make_synthetic_state_dict(R.RefConfig.from_dict(TINY), seed=3)
    m = StripedHyena(dict(TINY), ops=ops)
    m.load_state_dict({k: (v.double() if v.dtype == torch.bfloat16 else v) for k, v in sd.items()})
    return m


def test_a_backend_passes_through_and_a_duck_typed_object_is_adopted():
    ours, duck = OracleOps(torch.float64), _plain(OracleOps)(torch.float64)
    assert not isinstance(duck, Backend) and not hasattr(duck, "supports") and not hasattr(duck, "fuse_norm")
    assert Backend.adopt(ours) is ours and Backend.adopt(None) is None
    a = Backend.adopt(duck)
    assert isinstance(a, Backend) and a.name == "oracle-cpu" and a.act == torch.float64           # its own attributes win
    assert (a.fuse_norm, a.hyena_mfma, a.attn_prescale, a.hyena_table_guard, a.timer) == (False, False, False, True, None)
    assert not a.supports("hyena_ct") and not a.supports("rope_append_decode") and a.attn_q_scale(128) == Backend.attn_q_scale(128)
    a.timer = "t"                                                                                # writes reach the object itself
    assert duck.timer == "t" and a.timer == "t"


def test_the_forward_on_an_adopted_object_is_the_forward_on_the_backend():
    """Stateless forward, cached prefill, resumed prefill and decode steps: bit for bit what the Backend-derived oracle computes."""
    ids = torch.tensor([[0] + list(b"ACGTTGCAACGTAC"), [0] + list(b"GGGTTTACACGTAA")])
    outs = []
    for ops in (OracleOps(torch.float64), _plain(OracleOps)(torch.float64)):
        m = _model(ops)
        got = [m(ids)[0]]
        c = m.initialize_inference_params()
        c["mha"].max_batch_size = c["hyena"].max_batch_size = 2
        t = 0
        for n in (8, 4, 1, 1, 1):
            c["mha"].seqlen_offset = c["hyena"].seqlen_offset = t
            got.append(m(ids[:, t:t + n], c)[0])
            t += n
        outs.append(got)
    for x, y in zip(*outs):
        assert torch.equal(x, y)
    # a non-neutral value is still passed on -- and refused by a signature that does not know it
    a = Backend.adopt(_plain(OracleOps)(torch.float64))
    try:
        a.rope_(torch.zeros(1, 1, 3, 1, 2), torch.ones(1, 1), torch.zeros(1, 1), q_scale=0.5)
    except TypeError:
        pass
    else:
        raise AssertionError("q_scale = 0.5 was dropped")
