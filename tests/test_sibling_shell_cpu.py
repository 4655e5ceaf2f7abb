"""The siblings' shared Python shell (bsarec_amd/_sibling.py) without a GPU: the state_dict keys and shapes of the
eight model variants, in order, as the models had them before the shell existed (written out from that commit); the one layer
base and the one autograd node; and the flat-weight views after each of the three ways a parameter gets a new storage on a CPU."""
import argparse
import copy

import pytest
import torch

ARGS = dict(item_size=50, hidden_size=16, max_seq_length=12, num_hidden_layers=2, num_attention_heads=2, hidden_dropout_prob=0.1,
            attention_probs_dropout_prob=0.1, hidden_act="gelu", initializer_range=0.02, seed=1)

GRU_KEYS = [("item_embeddings.weight", (50, 16)), ("gru_layers.weight_ih_l0", (192, 16)), ("gru_layers.weight_hh_l0", (192, 64)),
            ("gru_layers.weight_ih_l1", (192, 64)), ("gru_layers.weight_hh_l1", (192, 64)), ("dense.weight", (16, 64)),
            ("dense.bias", (16,))]
CASER_CONV = [("conv.conv_v.weight", (4, 1, 12, 1)), ("conv.conv_v.bias", (4,)),
              ("conv.conv_h.0.weight", (16, 1, 1, 16)), ("conv.conv_h.0.bias", (16,)),
              ("conv.conv_h.1.weight", (16, 1, 2, 16)), ("conv.conv_h.1.bias", (16,)),
              ("conv.conv_h.2.weight", (16, 1, 3, 16)), ("conv.conv_h.2.bias", (16,)),
              ("conv.conv_h.3.weight", (16, 1, 4, 16)), ("conv.conv_h.3.bias", (16,)),
              ("conv.conv_h.4.weight", (16, 1, 5, 16)), ("conv.conv_h.4.bias", (16,)),
              ("conv.conv_h.5.weight", (16, 1, 6, 16)), ("conv.conv_h.5.bias", (16,)),
              ("conv.conv_h.6.weight", (16, 1, 7, 16)), ("conv.conv_h.6.bias", (16,)),
              ("conv.conv_h.7.weight", (16, 1, 8, 16)), ("conv.conv_h.7.bias", (16,)),
              ("conv.conv_h.8.weight", (16, 1, 9, 16)), ("conv.conv_h.8.bias", (16,)),
              ("conv.conv_h.9.weight", (16, 1, 10, 16)), ("conv.conv_h.9.bias", (16,)),
              ("conv.conv_h.10.weight", (16, 1, 11, 16)), ("conv.conv_h.10.bias", (16,)),
              ("conv.conv_h.11.weight", (16, 1, 12, 16)), ("conv.conv_h.11.bias", (16,)),
              ("fc1.weight", (16, 256)), ("fc1.bias", (16,))]
CASER_KEYS = [("item_embeddings.weight", (50, 16))] + CASER_CONV
CASER_USER_KEYS = ([("item_embeddings.weight", (50, 16)), ("user_embeddings.weight", (7, 16))] + CASER_CONV
                   + [("fc2.weight", (16, 32)), ("fc2.bias", (16,))])
FEED_FORWARD = [("feed_forward.dense_1.weight", (64, 16)), ("feed_forward.dense_1.bias", (64,)),
                ("feed_forward.dense_2.weight", (16, 64)), ("feed_forward.dense_2.bias", (16,)),
                ("feed_forward.LayerNorm.weight", (16,)), ("feed_forward.LayerNorm.bias", (16,))]
FEA_BLOCK = [("layer.query.weight", (16, 16)), ("layer.query.bias", (16,)), ("layer.key.weight", (16, 16)),
             ("layer.key.bias", (16,)), ("layer.value.weight", (16, 16)), ("layer.value.bias", (16,)),
             ("layer.dense.weight", (16, 16)), ("layer.dense.bias", (16,)), ("layer.LayerNorm.weight", (16,)),
             ("layer.LayerNorm.bias", (16,))] + FEED_FORWARD
LRU_BLOCK = [("lru.nu_log", (16,)), ("lru.theta_log", (16,)), ("lru.gamma_log", (16,)), ("lru.in_proj.weight", (32, 16)),
             ("lru.in_proj.bias", (32,)), ("lru.out_proj.weight", (16, 32)), ("lru.out_proj.bias", (16,)),
             ("lru.LayerNorm.weight", (16,)), ("lru.LayerNorm.bias", (16,))] + FEED_FORWARD
MAMBA_BLOCK = [("mamba.A_log", (32, 16)), ("mamba.D", (32,)), ("mamba.in_proj.weight", (64, 16)), ("mamba.conv1d.weight", (32, 4)),
               ("mamba.conv1d.bias", (32,)), ("mamba.x_proj.weight", (36, 32)), ("mamba.dt_proj.weight", (32, 4)),
               ("mamba.dt_proj.bias", (32,)), ("mamba.out_proj.weight", (16, 32)), ("mamba.LayerNorm.weight", (16,)),
               ("mamba.LayerNorm.bias", (16,))] + FEED_FORWARD


def _blocks(head, block):
    return head + [(f"item_encoder.blocks.{k}.{name}", shp) for k in (0, 1) for name, shp in block]


LN = [("LayerNorm.weight", (16,)), ("LayerNorm.bias", (16,))]
FEA_KEYS = _blocks([("item_embeddings.weight", (50, 16)), ("position_embeddings.weight", (12, 16))] + LN, FEA_BLOCK)
LRU_KEYS = _blocks([("item_embeddings.weight", (50, 16))] + LN, LRU_BLOCK)
MAMBA_KEYS = _blocks([("item_embeddings.weight", (50, 16))] + LN, MAMBA_BLOCK)

# (model class, extra args, keys and shapes, entries): the entry counts are the parent commit's 7, 7, 29, 32, 36, 33, 33, 37
VARIANTS = {"gru4rec": ("GRU4RecModel", {}, GRU_KEYS, 7),
            "gru4rec_fused": ("GRU4RecModel", dict(gru_step="fused"), GRU_KEYS, 7),
            "caser": ("CaserModel", {}, CASER_KEYS, 29),
            "caser_user_fused": ("CaserModel", dict(caser_step="fused", caser_user=True, num_users=7), CASER_USER_KEYS, 32),
            "fearec": ("FEARecModel", {}, FEA_KEYS, 36),
            "lrurec": ("LRURecModel", {}, LRU_KEYS, 33),
            "lrurec_fused": ("LRURecModel", dict(lru_step="fused"), LRU_KEYS, 33),
            "mamba4rec": ("Mamba4RecModel", {}, MAMBA_KEYS, 37)}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_state_dict_keys_and_shapes_are_the_parents(variant):
    import bsarec_amd
    cls, kw, want, count = VARIANTS[variant]
    torch.manual_seed(1)
    model = getattr(bsarec_amd, cls)(argparse.Namespace(**ARGS, **kw))
    got = [(k, tuple(v.shape)) for k, v in model.state_dict().items()]
    assert len(want) == count and got == want


def _layers():
    from bsarec_amd.caser import CaserConv
    from bsarec_amd.gru4rec import GruStack
    from bsarec_amd.lrurec import LruLayer
    from bsarec_amd.mamba4rec import MambaLayer
    return {"gru": lambda: GruStack(8, 32, 1, 8), "caser": lambda: CaserConv(12, 8, 4, 1), "lru": lambda: LruLayer(8),
            "mamba": lambda: MambaLayer(8, d_state=4, d_conv=2, expand=2, dt_rank=4)}


def test_one_layer_base_and_one_autograd_node(monkeypatch):
    from bsarec_amd import _sibling as S
    from bsarec_amd.fearec import FeaAttention
    layers = {name: make() for name, make in _layers().items()}
    layers["fea"] = FeaAttention(12, 8, 0, 7, 2)
    for name, layer in layers.items():
        assert isinstance(layer, S._KernelLayer), name
        assert isinstance(layer, S._FlatLayer) == (name != "fea"), name
    assert layers["fea"].flat_parameters() == [] and not layers["fea"]._slices

    # every forward reaches the same Function: on tensors that claim to be on the GPU, ``apply`` is the first thing to run
    seen = []

    class Probe:
        @staticmethod
        def apply(layer, extra, *tensors):
            seen.append((type(layer).__name__, len(tensors) - len(layer._slices)))
            return None

    monkeypatch.setattr(S, "_LayerFn", Probe)
    monkeypatch.setattr(torch.Tensor, "is_cuda", property(lambda self: True))
    x = torch.zeros(3, 12, 8, requires_grad=True)
    for name, layer in layers.items():
        layer(x, x, x) if name == "fea" else layer(x)
    assert seen == [("GruStack", 1), ("CaserConv", 1), ("LruLayer", 1), ("MambaLayer", 1), ("FeaAttention", 3)]
    subclasses = [c for c in vars(S).values() if isinstance(c, type) and issubclass(c, torch.autograd.Function)]
    assert len(subclasses) == 1


def _is_flat(layer):
    ps, base = layer.flat_parameters(), layer._flat
    assert len(ps) == len(layer._slices) and base.numel() == layer._numel and base.dtype == torch.float32
    for p, (o, n, shp) in zip(ps, layer._slices.values()):
        assert p.data_ptr() == base.data_ptr() + 4 * o and tuple(p.shape) == tuple(shp) and p.numel() == n
    return True


@pytest.mark.parametrize("name", ["gru", "caser", "lru", "mamba"])
def test_parameters_stay_views_of_the_flat_tensor(name):
    make = _layers()[name]
    torch.manual_seed(3)
    layer = make()
    assert _is_flat(layer)
    values = [p.detach().clone() for p in layer.flat_parameters()]
    flat = layer._flat

    twin = copy.deepcopy(layer)                              # deepcopy: new storages, one per parameter or one for all
    twin.reflatten()
    assert _is_flat(twin) and twin._flat.data_ptr() != flat.data_ptr()
    assert all(torch.equal(a, b) for a, b in zip(twin.flat_parameters(), values))

    layer.double().float()                                   # a dtype round trip: every parameter gets a storage of its own
    assert _is_flat(layer) and layer._flat is not flat and layer._pool == {}
    assert all(torch.equal(a, b) for a, b in zip(layer.flat_parameters(), values))

    torch.manual_seed(4)
    other = make()
    flat = layer._flat
    layer.load_state_dict(other.state_dict())                # copies in place: the views stay, the flat tensor has the values
    layer.reflatten()
    assert _is_flat(layer) and layer._flat is flat
    registered = dict(other.named_parameters())
    assert registered and all(torch.equal(p, registered[k]) for k, p in layer.named_parameters())
