"""What the host-side tests of the two block-model steps (test_lrurec_step_cpu.py, test_mamba4rec_step_cpu.py) share: the twin
of the model in torch double over a description T of the layer -- prefix and names(d) of its tensors, weights(rng, d) -> {name:
array}, layer(x, ids, {name: tensor}) in torch, and the reference (keys, ragged_ids, loss_and_grads, train_step) -- the three-step
comparison of the reference with it, and the mode switch with the flat weight array.  Not a test module: nothing is collected."""
import math

import numpy as np
import pytest

from oracle import bsarec_oracle as O

torch = pytest.importorskip("torch")


def random_params(T, rng, V, d, N):
    p = {"item_embeddings.weight": rng.normal(0, 0.5, (V, d))}
    for k in T.keys(N, d)[1:]:
        leaf = k.split(".")[-1]
        if f".{T.prefix}." in k and "LayerNorm" not in k:
            continue
        if "LayerNorm" in k:
            p[k] = (1.0 if leaf == "weight" else 0.0) + 0.1 * rng.normal(size=d)
        elif "dense_1" in k:
            p[k] = rng.normal(0, 1 / math.sqrt(d), (4 * d, d)) if leaf == "weight" else 0.1 * rng.normal(size=4 * d)
        else:
            p[k] = rng.normal(0, 1 / math.sqrt(4 * d), (d, 4 * d)) if leaf == "weight" else 0.1 * rng.normal(size=d)
    for k in range(N):
        for n, v in T.weights(rng, d).items():
            p[f"item_encoder.blocks.{k}.{T.prefix}.{n}"] = v.copy()
    return {k: p[k] for k in T.keys(N, d)}


def ln(x, w, b):
    xc = x - x.mean(-1, keepdim=True)
    return w * (xc / torch.sqrt((xc * xc).mean(-1, keepdim=True) + 1e-12)) + b


def twin_loss(T, tp, ids, answers, N, mults):
    """The model's _encode / calculate_loss in torch double, the dropout multipliers given."""
    E = tp["item_embeddings.weight"]
    d = E.shape[1]
    x = ln(E[ids], tp["LayerNorm.weight"], tp["LayerNorm.bias"]) * mults[0]
    for k in range(N):
        p = f"item_encoder.blocks.{k}."
        z = T.layer(x, ids, {n: tp[p + T.prefix + "." + n] for n in T.names(d)})
        a = ln(z * mults[1 + 2 * k] + x, tp[p + T.prefix + ".LayerNorm.weight"], tp[p + T.prefix + ".LayerNorm.bias"])
        f = a @ tp[p + "feed_forward.dense_1.weight"].T + tp[p + "feed_forward.dense_1.bias"]
        f = f * 0.5 * (1.0 + torch.erf(f / math.sqrt(2.0)))
        f = f @ tp[p + "feed_forward.dense_2.weight"].T + tp[p + "feed_forward.dense_2.bias"]
        x = ln(f * mults[2 + 2 * k] + a, tp[p + "feed_forward.LayerNorm.weight"], tp[p + "feed_forward.LayerNorm.bias"])
    return torch.nn.functional.cross_entropy(x[:, -1] @ E.T, answers)


def reference_equals_the_twin(T, shape, wd):
    """Three steps of the reference beside autograd and torch.optim.Adam on the twin, both in double, to 1e-12."""
    V, d, N, L, B = shape
    rng = np.random.default_rng(V)
    params = random_params(T, rng, V, d, N)
    first = list(rng.integers(0, L, B))
    first[0], first[1] = 0, L                                  # a full row, and a row of padding alone
    if B > 2:
        first[2] = L - 1                                       # a row whose first item is the last position
    ids = T.ragged_ids(rng, B, L, first, V)
    ans = rng.integers(1, V, B)
    ans[0] = ids[0, -1]                                        # a row that the lookup and the head both touch
    assert not ids[1].any() and ids[0].all() and (B <= 2 or (ids[2, :L - 1].sum() == 0 and ids[2, L - 1] != 0))
    tp = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in params.items()}
    # eps = 1e-3 in both optimisers: d(update) / d(g) is at most lr / eps, so the two gradients' last-bit differences (~1e-16)
    # stay far below the bound; at eps = 1e-8 a gradient element that happens to be near 0 multiplies them by up to 1e6
    opt = torch.optim.Adam(list(tp.values()), lr=1e-2, eps=1e-3, weight_decay=wd)
    st = O.AdamState(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-3, weight_decay=wd)
    tids, tans = torch.from_numpy(ids), torch.from_numpy(ans)
    for step in range(1, 4):
        mults = [(rng.random((B, L, d)) >= 0.5) * 2.0 for _ in range(1 + 2 * N)]       # explicit keep masks, p = 0.5
        rloss, rgrads, _ = T.loss_and_grads(params, ids, ans, N, mults)
        assert list(rgrads) == list(params) == T.keys(N, d)
        opt.zero_grad()
        loss = twin_loss(T, tp, tids, tans, N, [torch.from_numpy(m) for m in mults])
        loss.backward()
        assert abs(rloss - loss.item()) <= 1e-12
        for k, p in tp.items():
            assert rgrads[k].shape == p.shape and np.abs(rgrads[k] - p.grad.numpy()).max() <= 1e-12, (step, k)
        opt.step()
        assert T.train_step(params, st, ids, ans, N, mults) == rloss
        for k, p in tp.items():
            assert np.abs(params[k] - p.detach().numpy()).max() <= 1e-12, (step, k)
    assert st.t == 3


def mode_switch_and_the_flat_array(Model, args, flag, shapes, keys, layer, first, layer_floats):
    """``args(**kw)``: the file's argument builder (41 items, L = 6: the ids below); ``shapes``: the model's param shapes at
    args(); ``layer``: the block's attribute; ``first``: the layer's first tensor in the flat array; ``layer_floats``: the length
    of a layer's own array."""
    assert Model.torch_optim is True and Model.own_train_step is False
    torch.manual_seed(3)
    default = Model(args())
    torch.manual_seed(3)
    fused = Model(args(**{flag: "fused"}))
    torch_mode = Model(args(**{flag: "torch"}))
    assert getattr(default, flag) == getattr(torch_mode, flag) == "torch" and default.torch_optim is True
    assert torch_mode.torch_optim is True and default.own_train_step is False and default._wflat is None
    assert getattr(fused, flag) == "fused" and fused.torch_optim is False and fused.own_train_step is True
    assert fused.needs_negatives is False
    with pytest.raises(ValueError, match=flag + " must be 'torch' or 'fused'"):
        Model(args(**{flag: "bogus"}))
    # the same keys, shapes and (same seed) values in both modes; checkpoints pass between them
    sd, sf = default.state_dict(), fused.state_dict()
    assert list(sd) == list(sf) == keys
    for k in sd:
        assert sd[k].shape == sf[k].shape and torch.equal(sd[k], sf[k]), k
    with torch.no_grad():
        for q in fused.parameters():
            q.add_(0.25)
    torch_mode.load_state_dict(fused.state_dict())
    default.load_state_dict(torch_mode.state_dict())
    fused.load_state_dict(default.state_dict())

    def is_flat(m):
        flat, off = m._wflat, 0
        for (k, shp), q in zip(shapes.items(), m.flat_parameters()):
            if q.data_ptr() != flat.data_ptr() + 4 * off or tuple(q.shape) != shp or q is not dict(m.named_parameters())[k]:
                return False
            off += q.numel()
        for k, blk in enumerate(m.item_encoder.blocks):         # each layer's array is a slice of it, and the layer agrees
            la = getattr(blk, layer)
            o = m._wslices[f"item_encoder.blocks.{k}.{layer}.{first}"][0]
            if la._flat.data_ptr() != flat.data_ptr() + 4 * o or la._flat.numel() != layer_floats:
                return False
            held = la._flat
            la.reflatten()                                        # the pointer test accepts a slice: nothing is rebuilt
            if la._flat is not held:
                return False
        return off == flat.numel() and flat.data_ptr() % 16 == 0

    assert is_flat(fused)
    values = {k: v.clone() for k, v in fused.state_dict().items()}
    moved = fused.double().float()                                # gives every parameter a storage of its own, twice
    assert moved is fused and is_flat(fused)
    for k, v in fused.state_dict().items():
        assert torch.equal(v, values[k]), k
    ids = torch.randint(1, 41, (3, 6))
    with pytest.raises(RuntimeError, match="torch.optim.Adam"):
        default.train_step(ids, ids[:, 0])
    with pytest.raises(RuntimeError, match=flag + " = 'fused'"):
        default.loss_and_grads(ids, ids[:, 0])
    with pytest.raises(RuntimeError, match="MI355X"):               # no CPU path for the fused step either
        fused.train_step(ids, ids[:, 0])
    with pytest.raises(RuntimeError, match="MI355X"):
        fused.loss_and_grads(ids, ids[:, 0])
