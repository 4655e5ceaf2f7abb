"""numpy restatement of the linear recurrent unit layer (bsarec_lru_fwd / bsarec_lru_bwd, include/bsarec_hip.h), forward and
backward, in the dtype asked for (fp64: the reference; fp32: the plain restatement whose own error sizes a gate), and of the
whole LRURec model: its loss in numpy, and a torch twin in double whose recurrent layer is this restatement.  The layer's
backward is checked against torch's complex autograd in tests/test_lru_cpu.py."""
import math
from collections import OrderedDict

import numpy as np


def weight_shapes(d):
    return OrderedDict([("nu_log", (d,)), ("theta_log", (d,)), ("gamma_log", (d,)), ("in_proj.weight", (2 * d, d)),
                        ("in_proj.bias", (2 * d,)), ("out_proj.weight", (d, 2 * d)), ("out_proj.bias", (d,))])


def split_weights(flat, d):
    out, off = OrderedDict(), 0
    for k, shp in weight_shapes(d).items():
        n = int(np.prod(shp))
        out[k] = flat[off:off + n].reshape(shp)
        off += n
    assert off == flat.size == 4 * d * d + 6 * d
    return out


def flat_weights(w, d):
    return np.concatenate([np.asarray(w[k]).reshape(-1) for k in weight_shapes(d)])


def ring_init(rng, d, r_min=0.8, r_max=0.99):
    """nu_log, theta_log, gamma_log of the model's init, in double."""
    u1, u2 = rng.uniform(0, 1, d), rng.uniform(1e-3, 1, d)
    nu_log = np.log(-0.5 * np.log(u1 * (r_max ** 2 - r_min ** 2) + r_min ** 2))
    theta_log = np.log(2 * math.pi * u2)
    gamma_log = 0.5 * np.log(1.0 - np.exp(-2.0 * np.exp(nu_log)))
    return nu_log, theta_log, gamma_log


def random_weights(rng, d, r_min=0.8, r_max=0.99, nu_log=None):
    """fp32 flat weights: the ring init (or the given nu_log with its gamma_log), projections N(0, 1 / fan_in), biases N(0, 0.1)."""
    nu, th, ga = ring_init(rng, d, r_min, r_max)
    if nu_log is not None:
        nu = np.full(d, float(nu_log)) + rng.uniform(-0.05, 0.05, d)
        ga = 0.5 * np.log(1.0 - np.exp(-2.0 * np.exp(nu)))
    w = {"nu_log": nu, "theta_log": th, "gamma_log": ga,
         "in_proj.weight": rng.normal(0, 1 / math.sqrt(d), (2 * d, d)), "in_proj.bias": rng.normal(0, 0.1, 2 * d),
         "out_proj.weight": rng.normal(0, 1 / math.sqrt(2 * d), (d, 2 * d)), "out_proj.bias": rng.normal(0, 0.1, d)}
    return flat_weights(w, d).astype(np.float32)


def ragged_ids(rng, B, L, first=None, V=50):
    """Left-padded ids [B, L]: row b has its first item at first[b] (L: the row is padding alone); random starts when None."""
    ids = rng.integers(1, V, (B, L)).astype(np.int64)
    first = rng.integers(0, L, B) if first is None else first
    for b, f in enumerate(first):
        ids[b, :f] = 0
    return ids


def forward(x, ids, flat, dtype=np.float64):
    """y [B, L, d] and what the backward needs."""
    B, L, d = x.shape
    w = {k: v.astype(dtype) for k, v in split_weights(np.asarray(flat), d).items()}
    x = x.astype(dtype)
    m = (np.ones((B, L)) if ids is None else (ids != 0)).astype(dtype)[..., None]
    nu, th, gam = np.exp(w["nu_log"]), np.exp(w["theta_log"]), np.exp(w["gamma_log"])
    mag = np.exp(-nu)
    lr, li = mag * np.cos(th), mag * np.sin(th)
    u = x @ w["in_proj.weight"].T + w["in_proj.bias"]
    vr, vi = m * gam * u[..., :d], m * gam * u[..., d:]
    hr, hi = np.zeros((B, L, d), dtype), np.zeros((B, L, d), dtype)
    pr, pi = np.zeros((B, d), dtype), np.zeros((B, d), dtype)
    for t in range(L):
        pr, pi = lr * pr - li * pi + vr[:, t], lr * pi + li * pr + vi[:, t]
        hr[:, t], hi[:, t] = pr, pi
    h = np.concatenate([hr, hi], -1)
    y = h @ w["out_proj.weight"].T + w["out_proj.bias"]
    return y, dict(x=x, m=m, w=w, nu=nu, th=th, gam=gam, lr=lr, li=li, vr=vr, vi=vi, hr=hr, hi=hi, h=h, d=d, dtype=dtype)


def backward(c, dy):
    """dx [B, L, d] and the flat weight gradient."""
    d, dtype, w = c["d"], c["dtype"], c["w"]
    dy = dy.astype(dtype)
    B, L, _ = dy.shape
    lr, li, hr, hi, m, gam = c["lr"], c["li"], c["hr"], c["hi"], c["m"], c["gam"]
    g = dy @ w["out_proj.weight"]
    ar, ai = np.zeros((B, L, d), dtype), np.zeros((B, L, d), dtype)
    nr, ni = np.zeros((B, d), dtype), np.zeros((B, d), dtype)
    for t in range(L - 1, -1, -1):
        nr, ni = g[:, t, :d] + lr * nr + li * ni, g[:, t, d:] + lr * ni - li * nr
        ar[:, t], ai[:, t] = nr, ni
    lhr = (ar[:, 1:] * hr[:, :-1] + ai[:, 1:] * hi[:, :-1]).sum((0, 1))
    lhi = (ai[:, 1:] * hr[:, :-1] - ar[:, 1:] * hi[:, :-1]).sum((0, 1))
    zr, zi = lhr * lr + lhi * li, lhi * lr - lhr * li
    du = np.concatenate([m * gam * ar, m * gam * ai], -1)
    du2, dy2 = du.reshape(B * L, 2 * d), dy.reshape(B * L, d)
    dw = {"nu_log": -c["nu"] * zr, "theta_log": c["th"] * zi, "gamma_log": (ar * c["vr"] + ai * c["vi"]).sum((0, 1)),
          "in_proj.weight": du2.T @ c["x"].reshape(B * L, d), "in_proj.bias": du2.sum(0),
          "out_proj.weight": dy2.T @ c["h"].reshape(B * L, 2 * d), "out_proj.bias": dy2.sum(0)}
    return du @ w["in_proj.weight"], flat_weights(dw, d)


def torch_complex_layer(x, ids, w):
    """The layer on torch complex tensors with a Python loop over t, differentiable: ``w`` maps the seven names to tensors."""
    import torch
    B, L, d = x.shape
    m = torch.ones(B, L, dtype=x.dtype, device=x.device) if ids is None else (ids != 0).to(x.dtype)
    lam = torch.polar(torch.exp(-torch.exp(w["nu_log"])), torch.exp(w["theta_log"]))
    u = x @ w["in_proj.weight"].T + w["in_proj.bias"]
    v = (m[..., None] * torch.exp(w["gamma_log"])) * torch.complex(u[..., :d], u[..., d:])
    h, hs = torch.zeros(B, d, dtype=v.dtype, device=x.device), []
    for t in range(L):
        h = lam * h + v[:, t]
        hs.append(h)
    h = torch.stack(hs, 1)
    return torch.cat([h.real, h.imag], -1) @ w["out_proj.weight"].T + w["out_proj.bias"]


# ---- the whole model --------------------------------------------------------------------------------------------------------
def _ln(np_, x, w, b, sqrt):
    u = x.mean(-1, keepdims=True) if np_ is np else x.mean(-1, keepdim=True)
    xc = x - u
    s = (xc * xc).mean(-1, keepdims=True) if np_ is np else (xc * xc).mean(-1, keepdim=True)
    return w * (xc / sqrt(s + 1e-12)) + b


def layer_flat(sd, k):
    """The flat weight array of block k from a state_dict-like mapping of numpy arrays."""
    p = f"item_encoder.blocks.{k}.lru."
    d = sd[p + "nu_log"].shape[0]
    return flat_weights({n: sd[p + n] for n in weight_shapes(d)}, d)


def model_loss(sd, ids, answers, num_layers):
    """The model's loss and last-block output in numpy fp64 from a mapping name -> array (dropout 0)."""
    from scipy.special import erf
    sd = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
    E = sd["item_embeddings.weight"]
    x = _ln(np, E[ids], sd["LayerNorm.weight"], sd["LayerNorm.bias"], np.sqrt)
    for k in range(num_layers):
        p = f"item_encoder.blocks.{k}."
        z, _ = forward(x, ids, layer_flat(sd, k))
        a = _ln(np, z + x, sd[p + "lru.LayerNorm.weight"], sd[p + "lru.LayerNorm.bias"], np.sqrt)
        f = a @ sd[p + "feed_forward.dense_1.weight"].T + sd[p + "feed_forward.dense_1.bias"]
        f = f * 0.5 * (1.0 + erf(f / math.sqrt(2.0)))
        f = f @ sd[p + "feed_forward.dense_2.weight"].T + sd[p + "feed_forward.dense_2.bias"]
        x = _ln(np, f + a, sd[p + "feed_forward.LayerNorm.weight"], sd[p + "feed_forward.LayerNorm.bias"], np.sqrt)
    logits = x[:, -1] @ E.T
    mx = logits.max(1, keepdims=True)
    lse = np.log(np.exp(logits - mx).sum(1)) + mx[:, 0]
    return float((lse - logits[np.arange(len(answers)), answers]).mean()), x


def twin_forward(params, ids, num_layers):
    """The model in torch double on the CPU, differentiable in ``params`` (name -> double tensor); the recurrent layer is this
    file's ``forward`` / ``backward`` inside an autograd node.  Returns the last block's [B, L, d]."""
    import torch

    class Lru(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, *ws):
            d = x.shape[-1]
            flat = flat_weights({n: t.detach().numpy() for n, t in zip(weight_shapes(d), ws)}, d)
            y, ctx.cache = forward(x.detach().numpy(), ids_np, flat)
            return torch.from_numpy(y)

        @staticmethod
        def backward(ctx, gy):
            dx, dflat = backward(ctx.cache, gy.numpy())
            d = dx.shape[-1]
            return (torch.from_numpy(dx),) + tuple(torch.from_numpy(np.ascontiguousarray(v)) for v in split_weights(dflat, d).values())

    ids_np = ids.numpy() if hasattr(ids, "numpy") else np.asarray(ids)
    tids = torch.from_numpy(ids_np)
    E = params["item_embeddings.weight"]
    x = _ln(torch, E[tids], params["LayerNorm.weight"], params["LayerNorm.bias"], torch.sqrt)
    d = E.shape[1]
    for k in range(num_layers):
        p = f"item_encoder.blocks.{k}."
        z = Lru.apply(x, *[params[p + "lru." + n] for n in weight_shapes(d)])
        a = _ln(torch, z + x, params[p + "lru.LayerNorm.weight"], params[p + "lru.LayerNorm.bias"], torch.sqrt)
        f = a @ params[p + "feed_forward.dense_1.weight"].T + params[p + "feed_forward.dense_1.bias"]
        f = f * 0.5 * (1.0 + torch.erf(f / math.sqrt(2.0)))
        f = f @ params[p + "feed_forward.dense_2.weight"].T + params[p + "feed_forward.dense_2.bias"]
        x = _ln(torch, f + a, params[p + "feed_forward.LayerNorm.weight"], params[p + "feed_forward.LayerNorm.bias"], torch.sqrt)
    return x


def twin_loss(params, ids, answers, num_layers):
    import torch
    x = twin_forward(params, ids, num_layers)
    a = torch.as_tensor(np.asarray(answers), dtype=torch.int64)
    return torch.nn.functional.cross_entropy(x[:, -1] @ params["item_embeddings.weight"].T, a), x
