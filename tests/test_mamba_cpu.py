"""Mamba4Rec without a GPU: the fp64 restatement of the layer (mamba_ref) against torch's autograd of the same math in double,
the model's loss against its torch twin, the C ABI's host side (sizes, limits, symbols), the registration, the flags, the
state_dict, the init and the constructor's refusals."""
import argparse
import math
import os

import numpy as np
import pytest
import torch

import mamba_ref as R

NAMES = ("bsarec_mamba_weight_floats", "bsarec_mamba_workspace_bytes", "bsarec_mamba_fwd", "bsarec_mamba_bwd")
# (B, L, d, E, N, K)
SHAPES = [(1, 1, 4, 1, 4, 2), (3, 3, 16, 2, 16, 4), (5, 17, 100, 2, 16, 3)]


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    n = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / n) if n > 0 else float(np.linalg.norm(a - b))


@pytest.mark.parametrize("shape", SHAPES, ids=["-".join(map(str, s)) for s in SHAPES])
def test_restatement_equals_autograd_in_double(shape):
    B, L, d, E, N, K = shape
    hyper = (E, N, K, R.dt_rank(d))
    rng = np.random.default_rng(sum(shape))
    first = list(rng.integers(0, L, B))
    if B > 1:
        first[-1] = L                                                 # one row of padding alone
    ids = R.ragged_ids(rng, B, L, first)
    flat = R.random_weights(rng, d, *hyper).astype(np.float64)
    from bsarec_amd.mamba4rec import default_dt_rank, mamba_param_shapes
    assert flat.size == R.weight_floats(d, *hyper) and default_dt_rank(d) == hyper[3]
    assert list(mamba_param_shapes(d, E, N, K, hyper[3]).items()) == list(R.weight_shapes(d, *hyper).items())    # the library's layout
    x, dout = rng.normal(0, 1, (B, L, d)), rng.normal(0, 1, (B, L, d))
    for use_ids in (ids, None):
        out, cache = R.forward(x, use_ids, flat, hyper)
        dx, dflat = R.backward(cache, dout)
        w = {k: torch.from_numpy(np.array(v)).requires_grad_(True) for k, v in R.split_weights(flat, d, *hyper).items()}
        tx = torch.from_numpy(x).requires_grad_(True)
        tout = R.torch_layer(tx, None if use_ids is None else torch.from_numpy(use_ids), w, hyper)
        tout.backward(torch.from_numpy(dout))
        assert _rel(out, tout.detach().numpy()) <= 1e-10
        assert _rel(dx, tx.grad.numpy()) <= 1e-10
        got = R.split_weights(dflat, d, *hyper)
        for k in w:
            assert _rel(got[k], w[k].grad.numpy()) <= 1e-10, k
    # padding is a selection: out = 0 and dx = 0 at padded positions, and nothing at an item depends on x under the padding
    out, cache = R.forward(x, ids, flat, hyper)
    dx, dflat = R.backward(cache, dout)
    pad = ids == 0
    assert not out[pad].any() and not dx[pad].any()
    x2 = np.where(pad[..., None], 1e6, x)
    out2, cache2 = R.forward(x2, ids, flat, hyper)
    assert np.array_equal(out2, out)
    assert np.array_equal(R.backward(cache2, dout)[1], dflat)          # nor does any weight gradient
    if B > 1:                                                          # a batch of padding alone: every gradient is 0
        z = np.zeros((B, L), np.int64)
        o3, c3 = R.forward(x, z, flat, hyper)
        dx3, dw3 = R.backward(c3, dout)
        assert not o3.any() and not dx3.any() and not dw3.any()


def _ns(**kw):
    base = dict(item_size=50, hidden_size=16, max_seq_length=12, batch_size=4, hidden_dropout_prob=0.1,
                attention_probs_dropout_prob=0.1, num_hidden_layers=2, num_attention_heads=2, hidden_act="gelu",
                initializer_range=0.02, seed=1)
    base.update(kw)
    return argparse.Namespace(**base)


def test_model_loss_equals_the_torch_twin():
    from bsarec_amd.mamba4rec import Mamba4RecModel
    torch.manual_seed(3)
    m = Mamba4RecModel(_ns(hidden_dropout_prob=0.0, mamba_d_state=8, mamba_d_conv=3))
    hyper = (2, 8, 3, 4)
    sd = {k: v.detach().double() for k, v in m.state_dict().items()}
    rng = np.random.default_rng(5)
    ids = R.ragged_ids(rng, 4, 12)
    answers = rng.integers(1, 50, 4)
    loss, x = R.model_loss({k: v.numpy() for k, v in sd.items()}, ids, answers, 2, hyper)
    tl, tx = R.twin_loss({k: v.clone().requires_grad_(True) for k, v in sd.items()}, ids, answers, 2, hyper)
    assert abs(loss - tl.item()) <= 1e-10 * abs(loss) and _rel(x, tx.detach().numpy()) <= 1e-10
    tl.backward()                                                     # the twin differentiates


def test_symbols_sizes_and_limits():
    from bsarec_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes == _lib.EXPORTS[name][1]
        assert getattr(lib, name).restype == _lib.EXPORTS[name][0]
    assert [f[0] for f in _lib.MambaConfig._fields_] == ["batch", "seq_len", "width", "expand", "d_state", "d_conv", "dt_rank"]
    assert lib.bsarec_abi_version() == 10 and _lib.ABI_VERSION == 10
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "bsarec_hip.h")).read()
    for name in NAMES + ("bsarec_mamba_config_t",):
        assert name in header
    cfg = _lib.MambaConfig
    for B, Lq, d, E, N, K, Rk in ((1, 1, 4, 1, 4, 2, 4), (5, 50, 64, 2, 16, 4, 4), (256, 50, 64, 2, 16, 4, 4),
                                  (65536, 256, 256, 2, 32, 4, 64), (3, 7, 100, 2, 8, 3, 8)):
        c = cfg(B, Lq, d, E, N, K, Rk)
        di = E * d
        floats = lib.bsarec_mamba_weight_floats(c)
        assert floats == R.weight_floats(d, E, N, K, Rk) == 3 * di * d + di * (K + 3 + Rk + N) + (Rk + 2 * N) * di
        off = 0
        for shp in R.weight_shapes(d, E, N, K, Rk).values():             # every tensor at a multiple of 4 floats
            assert off % 4 == 0
            off += int(np.prod(shp))
        ev, tr = lib.bsarec_mamba_workspace_bytes(c, 0), lib.bsarec_mamba_workspace_bytes(c, 1)
        assert 0 < ev <= tr and ev % 16 == 0 and tr % 16 == 0
        assert ev >= 4 * B * Lq * 5 * di
    buf = np.zeros(1 << 16, np.float32)
    p16 = (buf.ctypes.data + 63) & ~15
    ok = cfg(2, 5, 8, 2, 4, 2, 4)
    big = lib.bsarec_mamba_workspace_bytes(ok, 1)
    nx, nw = 4 * 2 * 5 * 8, 4 * lib.bsarec_mamba_weight_floats(ok)
    assert nw > 0 and 4 * nx + 2 * nw + big + 256 < buf.nbytes
    # distinct spans: x, weights, out / dout, dx, dweights, workspace
    px, pw, po, pdx, pdw = p16, p16 + nx, p16 + nx + nw, p16 + 2 * nx + nw, p16 + 3 * nx + nw
    pws = p16 + 3 * nx + 2 * nw

    def fwd(c, x=px, w=pw, y=po, ws=pws, n=big):
        return lib.bsarec_mamba_fwd(c, x, None, w, 1, y, ws, n, None)

    def bwd(c, x=px, w=pw, dy=po, ws=pws, n=big, dx=pdx, dw=pdw):
        return lib.bsarec_mamba_bwd(c, x, None, w, dy, ws, n, dx, dw, None)

    good = (2, 5, 8, 2, 4, 2, 4)
    bad_values = {0: (0, 65537), 1: (0, 257), 2: (0, 2, 6, 260), 3: (0, 3), 4: (0, 2, 12, 64), 5: (1, 5), 6: (0, 2, 6, 68)}
    for field, values in bad_values.items():
        for v in values:
            t = list(good)
            t[field] = v
            c = cfg(*t)
            assert lib.bsarec_mamba_weight_floats(c) < 0 and lib.bsarec_mamba_workspace_bytes(c, 0) < 0, t
            assert lib.bsarec_mamba_workspace_bytes(c, 1) < 0 and fwd(c) < 0 and bwd(c) < 0, t
    assert lib.bsarec_mamba_weight_floats(None) < 0 and lib.bsarec_mamba_workspace_bytes(None, 1) < 0
    assert fwd(None) < 0 and bwd(None) < 0
    # pointers: null, misaligned; the workspace size; aliasing -- all refused before any HIP call
    for kw in (dict(x=None), dict(w=None), dict(y=None), dict(ws=None), dict(x=px + 4), dict(w=pw + 4), dict(y=po + 4),
               dict(ws=pws + 4), dict(n=big - 1), dict(n=0), dict(y=px), dict(y=pw), dict(y=pws), dict(y=pws + big - 16),
               dict(ws=px), dict(ws=pw)):
        assert fwd(ok, **kw) < 0, kw
    for kw in (dict(x=None), dict(w=None), dict(dy=None), dict(ws=None), dict(dx=None), dict(dw=None), dict(x=px + 4),
               dict(w=pw + 4), dict(dy=po + 4), dict(ws=pws + 4), dict(dx=pdx + 4), dict(dw=pdw + 4), dict(n=big - 1),
               dict(dx=px), dict(dx=po), dict(dx=pw), dict(dx=pws), dict(dw=pw), dict(dw=px), dict(dw=pdx), dict(dw=pws),
               dict(ws=po)):
        assert bwd(ok, **kw) < 0, kw
    # the evaluation workspace does not serve a training call
    assert lib.bsarec_mamba_fwd(ok, px, None, pw, 1, po, pws, lib.bsarec_mamba_workspace_bytes(ok, 0), None) < 0


def test_registration_and_flags():
    import bsarec_amd
    from bsarec_amd import Mamba4RecModel, MambaLayer, main as M
    from bsarec_amd.mamba4rec import Mamba4RecModel as M2, default_dt_rank
    assert Mamba4RecModel is M2 and M.MODEL_REGISTRY["mamba4rec"] is Mamba4RecModel
    assert M.model_class("Mamba4Rec") is Mamba4RecModel and M.model_class("mamba4rec") is Mamba4RecModel
    assert "Mamba4RecModel" in bsarec_amd.__all__ and "MambaLayer" in bsarec_amd.__all__ and MambaLayer is not None
    assert "lrurec" in M.MODEL_REGISTRY and "mamba4rec" not in M.MODEL_DICT and "mamba4rec" not in M.SIBLING_MODELS
    flags = ("mamba_d_state", "mamba_d_conv", "mamba_expand", "mamba_dt_rank")
    a = M.parse_args([])
    assert not any(hasattr(a, f) for f in flags)
    a = M.parse_args(["--model_type", "Mamba4Rec", "--mamba_d_state", "8", "--mamba_d_conv", "3", "--mamba_expand", "1",
                      "--mamba_dt_rank", "12"])
    assert [getattr(a, f) for f in flags] == [8, 3, 1, 12]
    for argv in (["--mamba_d_state", "0"], ["--mamba_d_state", "12"], ["--mamba_d_state", "64"], ["--mamba_d_state", "x"],
                 ["--mamba_d_conv", "1"], ["--mamba_d_conv", "5"], ["--mamba_expand", "0"], ["--mamba_expand", "3"],
                 ["--mamba_expand", "1.5"], ["--mamba_dt_rank", "0"], ["--mamba_dt_rank", "6"], ["--mamba_dt_rank", "68"]):
        with pytest.raises(SystemExit):
            M.parse_args(argv)
    assert [default_dt_rank(d) for d in (4, 64, 68, 128, 256)] == [4, 4, 8, 8, 16]
    m = Mamba4RecModel(_ns(hidden_size=128, num_hidden_layers=1))
    la = m.item_encoder.blocks[0].mamba
    assert (la.d_state, la.d_conv, la.expand, la.dt_rank) == (16, 4, 2, 8)


def test_state_dict_views_and_init():
    from bsarec_amd.mamba4rec import Mamba4RecModel, MambaLayer, mamba_param_shapes
    torch.manual_seed(0)
    d, V, N = 16, 50, 2
    hyper = (2, 16, 4, 4)                                              # E, N, K, R: the defaults at d = 16
    m = Mamba4RecModel(_ns())
    want = {"item_embeddings.weight": (V, d), "LayerNorm.weight": (d,), "LayerNorm.bias": (d,)}
    for k in range(N):
        p = f"item_encoder.blocks.{k}."
        want.update({p + "mamba." + n: s for n, s in R.weight_shapes(d, *hyper).items()})
        want.update({p + "mamba.LayerNorm.weight": (d,), p + "mamba.LayerNorm.bias": (d,),
                     p + "feed_forward.dense_1.weight": (4 * d, d), p + "feed_forward.dense_1.bias": (4 * d,),
                     p + "feed_forward.dense_2.weight": (d, 4 * d), p + "feed_forward.dense_2.bias": (d,),
                     p + "feed_forward.LayerNorm.weight": (d,), p + "feed_forward.LayerNorm.bias": (d,)})
    sd = m.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == want
    assert len(list(m.parameters())) == len(want)
    shapes = mamba_param_shapes(d, 2, 16, 4, 4)
    assert list(shapes) == list(R.weight_shapes(d, *hyper)) and dict(shapes) == dict(R.weight_shapes(d, *hyper))
    # the nine tensors of a block are views of one flat tensor in the ABI's order, and stay so across load_state_dict and .to()
    for blk in m.item_encoder.blocks:
        la = blk.mamba
        assert la._flat.numel() == R.weight_floats(d, *hyper)
        assert torch.equal(torch.cat([p.detach().reshape(-1) for p in la.flat_parameters()]), la._flat)
        assert all(p.data_ptr() == la._flat.data_ptr() + 4 * o for p, (o, n, s) in zip(la.flat_parameters(), la._slices.values()))
        assert all(o % 4 == 0 for o, n, s in la._slices.values())
    torch.manual_seed(1)
    other = Mamba4RecModel(_ns())
    other.load_state_dict(sd)
    m.double().float()
    for a, b in zip(m.item_encoder.blocks, other.item_encoder.blocks):
        assert torch.equal(a.mamba._flat, b.mamba._flat)
        assert all(p.data_ptr() == a.mamba._flat.data_ptr() + 4 * o
                   for p, (o, n, s) in zip(a.mamba.flat_parameters(), a.mamba._slices.values()))
        assert len({p.untyped_storage().data_ptr() for p in a.mamba.flat_parameters()}) == 1
    with torch.no_grad():                                              # an in-place update of a view is an update of the array
        other.item_encoder.blocks[0].mamba.out_proj.weight.add_(1.0)
    la, lb = other.item_encoder.blocks[0].mamba, m.item_encoder.blocks[0].mamba
    assert torch.equal(la._flat[-d * 2 * d:], lb._flat[-d * 2 * d:] + 1.0)
    # init
    for K, Rk, Ns in ((4, 16, 16), (2, 4, 32), (3, 64, 4)):
        la = MambaLayer(256, Ns, K, 2, Rk, 0.02)
        di = 512
        for name in ("in_proj", "x_proj", "out_proj"):
            assert 0.018 < getattr(la, name).weight.std().item() < 0.022 and not hasattr(getattr(la, name), "bias")
        for t in (la.conv1d.weight, la.conv1d.bias):
            assert t.abs().max().item() <= K ** -0.5 and t.abs().max().item() > 0.9 * K ** -0.5
        assert la.conv1d.weight.shape == (di, K) and la.dt_proj.weight.shape == (di, Rk)
        assert la.dt_proj.weight.abs().max().item() <= Rk ** -0.5 and la.dt_proj.weight.abs().max().item() > 0.9 * Rk ** -0.5
        dt = torch.nn.functional.softplus(la.dt_proj.bias.detach().double())
        assert (dt >= 1e-3 * (1 - 1e-4)).all() and (dt <= 1e-1 * (1 + 1e-4)).all() and dt.max() / dt.min() > 10
        assert torch.allclose(la.A_log.detach(), torch.log(torch.arange(1, Ns + 1.0)).expand(di, Ns))
        assert (la.D == 1).all()
    assert abs(m.item_embeddings.weight.std().item() - 0.02) < 0.005
    ff = m.item_encoder.blocks[0].feed_forward
    assert not ff.dense_1.bias.any() and 0.015 < ff.dense_1.weight.std().item() < 0.025


def test_interface_and_refusals():
    from bsarec_amd.mamba4rec import Mamba4RecModel, MambaLayer
    assert (Mamba4RecModel.needs_negatives, Mamba4RecModel.needs_same_target, Mamba4RecModel.torch_optim) == (False, False, True)
    assert Mamba4RecModel.full_logits is None and Mamba4RecModel.kernel_family == "Mamba"
    m = Mamba4RecModel(_ns())
    for name in ("forward", "predict", "last_hidden", "catalogue_weight", "calculate_loss", "set_seed", "check_trainer"):
        assert callable(getattr(m, name))
    assert m._ce_pool == {}
    m.check_trainer(_ns(), None)
    with pytest.raises(ValueError, match="Mamba4Rec: single GPU only"):
        m.check_trainer(_ns(), object())
    for kw, msg in ((dict(storage="bf16"), "Mamba4Rec: storage = 'bf16'"), (dict(plan_options={"storage": 1}), "Mamba4Rec: storage"),
                    (dict(train_negatives=8), "Mamba4Rec: train_negatives"), (dict(train_lazy_adam=True), "Mamba4Rec: train_lazy_adam"),
                    (dict(mamba_d_state=12), "Mamba4Rec: mamba_d_state"), (dict(mamba_d_conv=5), "Mamba4Rec: mamba_d_conv"),
                    (dict(mamba_expand=3), "Mamba4Rec: mamba_expand"), (dict(mamba_dt_rank=6), "Mamba4Rec: mamba_dt_rank"),
                    (dict(mamba_dt_rank=68), "Mamba4Rec: mamba_dt_rank"), (dict(hidden_size=6), "Mamba4Rec: hidden_size"),
                    (dict(hidden_size=260), "Mamba4Rec: hidden_size"), (dict(num_hidden_layers=0), "Mamba4Rec: num_hidden_layers")):
        with pytest.raises(ValueError, match=msg):
            Mamba4RecModel(_ns(**kw))
    ids = torch.ones(2, 12, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="MI355X only"):
        m(ids)
    with pytest.raises(RuntimeError, match="MI355X only"):
        m.last_hidden(ids)
    with pytest.raises(RuntimeError, match="MI355X only"):
        MambaLayer(16)(torch.zeros(2, 12, 16))
    with pytest.raises(RuntimeError, match="calculate_loss"):
        m.grad_step(ids, ids[:, 0])
