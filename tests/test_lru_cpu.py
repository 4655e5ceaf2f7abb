"""LRURec without a GPU: the fp64 restatement of the layer (lru_ref) against torch's complex autograd, the C ABI's host side
(sizes, limits, symbols), the registration, the flags, the state_dict, the init and the constructor's refusals."""
import argparse
import math
import os

import numpy as np
import pytest
import torch

import lru_ref as R

NAMES = ("bsarec_lru_weight_floats", "bsarec_lru_workspace_bytes", "bsarec_lru_fwd", "bsarec_lru_bwd")
SHAPES = [(3, 7, 4), (2, 1, 8), (4, 20, 12)]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / n) if n > 0 else float(np.linalg.norm(a - b))


@pytest.mark.parametrize("shape", SHAPES, ids=["-".join(map(str, s)) for s in SHAPES])
def test_restatement_equals_complex_autograd_in_double(shape):
    B, L, d = shape
    rng = np.random.default_rng(B * 100 + L * 10 + d)
    first = list(rng.integers(0, L, B))
    first[-1] = L                                                     # one row of padding alone
    ids = R.ragged_ids(rng, B, L, first)
    flat = R.random_weights(rng, d).astype(np.float64)
    x, dy = rng.normal(0, 1, (B, L, d)), rng.normal(0, 1, (B, L, d))
    y, cache = R.forward(x, ids, flat)
    dx, dflat = R.backward(cache, dy)

    w = {k: torch.from_numpy(np.array(v)).requires_grad_(True) for k, v in R.split_weights(flat, d).items()}
    tx = torch.from_numpy(x).requires_grad_(True)
    ty = R.torch_complex_layer(tx, torch.from_numpy(ids), w)
    ty.backward(torch.from_numpy(dy))
    assert _rel(y, ty.detach().numpy()) <= 1e-12
    assert _rel(dx, tx.grad.numpy()) <= 1e-12
    got = R.split_weights(dflat, d)
    for k in w:
        ref = w[k].grad.numpy()
        if L == 1 and k in ("nu_log", "theta_log"):
            assert not got[k].any() and not ref.any()                 # no t >= 1: exactly zero
        else:
            assert _rel(got[k], ref) <= 1e-12, k
    # padding: h = 0 and y = out_proj.bias on the padded row, dx = 0 there, and nothing real depends on x under the padding
    ws = R.split_weights(flat, d)
    assert np.array_equal(y[-1], np.broadcast_to(ws["out_proj.bias"], (L, d))) and not dx[-1].any()
    x2 = np.where((ids == 0)[..., None], 1e6, x)
    y2, _ = R.forward(x2, ids, flat)
    assert np.array_equal(y2[ids != 0], y[ids != 0])
    # ids = None is the unmasked layer
    y3, c3 = R.forward(x, None, flat)
    ty3 = R.torch_complex_layer(torch.from_numpy(x), None, {k: v.detach() for k, v in w.items()})
    assert _rel(y3, ty3.numpy()) <= 1e-12


def test_model_loss_equals_the_torch_twin():
    from bsarec_amd.lrurec import LRURecModel
    torch.manual_seed(3)
    m = LRURecModel(_ns(hidden_dropout_prob=0.0))
    sd = {k: v.detach().double() for k, v in m.state_dict().items()}
    rng = np.random.default_rng(5)
    ids = R.ragged_ids(rng, 4, 12)
    answers = rng.integers(1, 50, 4)
    loss, x = R.model_loss({k: v.numpy() for k, v in sd.items()}, ids, answers, 2)
    tl, tx = R.twin_loss({k: v.clone().requires_grad_(True) for k, v in sd.items()}, ids, answers, 2)
    assert abs(loss - tl.item()) <= 1e-12 * abs(loss) and _rel(x, tx.detach().numpy()) <= 1e-12
    tl.backward()                                                     # the twin's node differentiates


def test_symbols_sizes_and_limits():
    from bsarec_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes == _lib.EXPORTS[name][1]
        assert getattr(lib, name).restype == _lib.EXPORTS[name][0]
    assert [f[0] for f in _lib.LruConfig._fields_] == ["batch", "seq_len", "width"]
    assert lib.bsarec_abi_version() == 10 and _lib.ABI_VERSION == 10
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "bsarec_hip.h")).read()
    for name in NAMES + ("bsarec_lru_config_t",):
        assert name in header
    cfg = _lib.LruConfig
    for B, Lq, d in ((1, 1, 4), (5, 50, 64), (256, 50, 64), (65536, 256, 256), (3, 7, 100)):
        assert lib.bsarec_lru_weight_floats(cfg(B, Lq, d)) == 4 * d * d + 6 * d
        ev, tr = lib.bsarec_lru_workspace_bytes(cfg(B, Lq, d), 0), lib.bsarec_lru_workspace_bytes(cfg(B, Lq, d), 1)
        assert 0 < ev <= tr and ev % 16 == 0 and tr % 16 == 0
        assert ev >= 4 * 2 * B * Lq * 2 * d and tr >= 4 * 3 * B * Lq * 2 * d          # v and h; and g in training
    buf = np.zeros(4096, np.float32)
    p16 = (buf.ctypes.data + 63) & ~15
    ok = cfg(5, 50, 64)
    big = lib.bsarec_lru_workspace_bytes(ok, 1)
    fwd = lambda c, x=p16, w=p16, y=p16, ws=p16, n=big: lib.bsarec_lru_fwd(c, x, None, w, 1, y, ws, n, None)
    bwd = lambda c, x=p16, w=p16, dy=p16, ws=p16, n=big, dx=p16, dw=p16: lib.bsarec_lru_bwd(c, x, None, w, dy, ws, n, dx, dw, None)
    for bad in ((5, 0, 64), (5, 257, 64), (5, 50, 2), (5, 50, 6), (5, 50, 260), (5, 50, 0), (0, 50, 64), (65537, 50, 64)):
        c = cfg(*bad)
        assert lib.bsarec_lru_weight_floats(c) < 0 and lib.bsarec_lru_workspace_bytes(c, 0) < 0, bad
        assert lib.bsarec_lru_workspace_bytes(c, 1) < 0 and fwd(c) < 0 and bwd(c) < 0, bad
    assert lib.bsarec_lru_weight_floats(None) < 0 and lib.bsarec_lru_workspace_bytes(None, 1) < 0
    assert fwd(None) < 0 and bwd(None) < 0
    # pointers: null, misaligned; the workspace size -- all refused before any HIP call
    for kw in (dict(x=None), dict(w=None), dict(y=None), dict(ws=None), dict(x=p16 + 4), dict(w=p16 + 4), dict(y=p16 + 4),
               dict(ws=p16 + 4), dict(n=big - 1), dict(n=0)):
        assert fwd(ok, **kw) < 0, kw
    for kw in (dict(x=None), dict(w=None), dict(dy=None), dict(ws=None), dict(dx=None), dict(dw=None), dict(x=p16 + 4),
               dict(w=p16 + 4), dict(dy=p16 + 4), dict(ws=p16 + 4), dict(dx=p16 + 4), dict(dw=p16 + 4), dict(n=big - 1)):
        assert bwd(ok, **kw) < 0, kw
    # the evaluation workspace does not serve a training call
    assert lib.bsarec_lru_fwd(ok, p16, None, p16, 1, p16, p16, lib.bsarec_lru_workspace_bytes(ok, 0), None) < 0


def _ns(**kw):
    base = dict(item_size=50, hidden_size=16, max_seq_length=12, batch_size=4, hidden_dropout_prob=0.1,
                attention_probs_dropout_prob=0.1, num_hidden_layers=2, num_attention_heads=2, hidden_act="gelu",
                initializer_range=0.02, seed=1)
    base.update(kw)
    return argparse.Namespace(**base)


def test_registration_and_flags():
    import bsarec_amd
    from bsarec_amd import LRURecModel, LruLayer, main as M
    from bsarec_amd.lrurec import LRURecModel as M2
    assert LRURecModel is M2 and M.MODEL_REGISTRY["lrurec"] is LRURecModel
    assert M.model_class("LRURec") is LRURecModel and M.model_class("lrurec") is LRURecModel
    assert "LRURecModel" in bsarec_amd.__all__ and "LruLayer" in bsarec_amd.__all__ and LruLayer is not None
    assert "fearec" in M.MODEL_REGISTRY and "lrurec" not in M.MODEL_DICT and "lrurec" not in M.SIBLING_MODELS
    a = M.parse_args([])
    assert not hasattr(a, "lru_r_min") and not hasattr(a, "lru_r_max")
    a = M.parse_args(["--model_type", "LRURec", "--lru_r_min", "0.5", "--lru_r_max", "0.9"])
    assert (a.lru_r_min, a.lru_r_max) == (0.5, 0.9)
    assert M.parse_args(["--lru_r_min", "0"]).lru_r_min == 0.0
    for argv in (["--lru_r_min", "-0.1"], ["--lru_r_min", "1"], ["--lru_r_max", "1"], ["--lru_r_max", "nan"], ["--lru_r_min", "x"],
                 ["--lru_r_min", "0.9", "--lru_r_max", "0.9"], ["--lru_r_min", "0.995"], ["--lru_r_max", "0.5"]):
        with pytest.raises(SystemExit):
            M.parse_args(argv)


def test_state_dict_views_and_init():
    from bsarec_amd.lrurec import LRURecModel, LruLayer, lru_param_shapes
    torch.manual_seed(0)
    d, V, N = 16, 50, 2
    m = LRURecModel(_ns())
    want = {"item_embeddings.weight": (V, d), "LayerNorm.weight": (d,), "LayerNorm.bias": (d,)}
    for k in range(N):
        p = f"item_encoder.blocks.{k}."
        want.update({p + "lru." + n: s for n, s in lru_param_shapes(d).items()})
        want.update({p + "lru.LayerNorm.weight": (d,), p + "lru.LayerNorm.bias": (d,),
                     p + "feed_forward.dense_1.weight": (4 * d, d), p + "feed_forward.dense_1.bias": (4 * d,),
                     p + "feed_forward.dense_2.weight": (d, 4 * d), p + "feed_forward.dense_2.bias": (d,),
                     p + "feed_forward.LayerNorm.weight": (d,), p + "feed_forward.LayerNorm.bias": (d,)})
    sd = m.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert len(list(m.parameters())) == len(want)
    assert list(lru_param_shapes(d)) == list(R.weight_shapes(d)) and dict(lru_param_shapes(d)) == dict(R.weight_shapes(d))
    # the seven tensors of a block are views of one flat tensor in the ABI's order, and stay so across load_state_dict and .to()
    for blk in m.item_encoder.blocks:
        la = blk.lru
        assert la._flat.numel() == 4 * d * d + 6 * d
        assert torch.equal(torch.cat([p.detach().reshape(-1) for p in la.flat_parameters()]), la._flat)
        assert all(p.data_ptr() == la._flat.data_ptr() + 4 * o for p, (o, n, s) in zip(la.flat_parameters(), la._slices.values()))
    torch.manual_seed(1)
    other = LRURecModel(_ns())
    other.load_state_dict(sd)
    m.double().float()
    for a, b in zip(m.item_encoder.blocks, other.item_encoder.blocks):
        assert torch.equal(a.lru._flat, b.lru._flat)
        assert all(p.data_ptr() == a.lru._flat.data_ptr() + 4 * o
                   for p, (o, n, s) in zip(a.lru.flat_parameters(), a.lru._slices.values()))
    with torch.no_grad():                                              # an in-place update of a view is an update of the array
        other.item_encoder.blocks[0].lru.out_proj.bias.add_(1.0)
    assert torch.equal(other.item_encoder.blocks[0].lru._flat[-d:], torch.ones(d))
    # init: |lambda| inside the ring, gamma_log = log sqrt(1 - |lambda|^2), projections N(0, std), biases 0
    for r_min, r_max in ((0.8, 0.99), (0.0, 0.5), (0.3, 0.31)):
        la = LruLayer(256, r_min, r_max, 0.02)
        mod = torch.exp(-torch.exp(la.nu_log.detach().double()))
        assert (mod >= r_min - 1e-6).all() and (mod <= r_max + 1e-6).all()
        assert torch.allclose(la.gamma_log.detach().double(), 0.5 * torch.log(1 - mod * mod), rtol=1e-5, atol=1e-6)
        th = torch.exp(la.theta_log.detach())
        assert (th >= 0).all() and (th <= 2 * math.pi * (1 + 1e-6)).all()
        assert not la.in_proj.bias.any() and not la.out_proj.bias.any()
        assert 0.015 < la.in_proj.weight.std().item() < 0.025 and 0.015 < la.out_proj.weight.std().item() < 0.025
    lam = m.item_encoder.blocks[0].lru
    mod = torch.exp(-torch.exp(lam.nu_log.detach()))
    assert (mod >= 0.8 - 1e-6).all() and (mod <= 0.99 + 1e-6).all()
    assert abs(m.item_embeddings.weight.std().item() - 0.02) < 0.005


def test_interface_and_refusals():
    from bsarec_amd.lrurec import LRURecModel, LruLayer
    assert (LRURecModel.needs_negatives, LRURecModel.needs_same_target, LRURecModel.torch_optim) == (False, False, True)
    assert LRURecModel.full_logits is None and LRURecModel.kernel_family == "LRU"
    m = LRURecModel(_ns())
    for name in ("forward", "predict", "last_hidden", "catalogue_weight", "calculate_loss", "set_seed", "check_trainer"):
        assert callable(getattr(m, name))
    assert m._ce_pool == {}
    m.check_trainer(_ns(), None)
    with pytest.raises(ValueError, match="LRURec: single GPU only"):
        m.check_trainer(_ns(), object())
    for kw, msg in ((dict(storage="bf16"), "LRURec: storage = 'bf16'"), (dict(plan_options={"storage": 1}), "LRURec: storage"),
                    (dict(train_negatives=8), "LRURec: train_negatives"), (dict(train_lazy_adam=True), "LRURec: train_lazy_adam"),
                    (dict(lru_r_min=0.9, lru_r_max=0.9), "LRURec: lru_r_min"), (dict(lru_r_max=1.0), "LRURec: lru_r_min"),
                    (dict(lru_r_min=-0.1), "LRURec: lru_r_min"), (dict(hidden_size=6), "LRURec: hidden_size"),
                    (dict(hidden_size=260), "LRURec: hidden_size"), (dict(num_hidden_layers=0), "LRURec: num_hidden_layers")):
        with pytest.raises(ValueError, match=msg):
            LRURecModel(_ns(**kw))
    ids = torch.ones(2, 12, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="MI355X only"):
        m(ids)
    with pytest.raises(RuntimeError, match="MI355X only"):
        LruLayer(16)(torch.zeros(2, 12, 16))
    with pytest.raises(RuntimeError, match="calculate_loss"):
        m.train_step(ids, ids[:, 0])
