"""numpy restatement in double of the selective state-space layer (bsarec_mamba_fwd / bsarec_mamba_bwd, include/bsarec_hip.h),
forward and a hand-written backward, the same layer in differentiable torch ops (a Python loop over t), and the whole Mamba4Rec
model: its loss in numpy and a torch twin in double.  The hand-written backward is checked against torch's autograd of the torch
layer in tests/test_mamba_cpu.py."""
import math
from collections import OrderedDict

import numpy as np

from lru_ref import _ln, ragged_ids  # noqa: F401  (ragged_ids: left-padded ids [B, L], row b's first item at first[b])


def weight_shapes(d, E, N, K, R):
    di = E * d
    return OrderedDict([("in_proj.weight", (2 * di, d)), ("conv1d.weight", (di, K)), ("conv1d.bias", (di,)),
                        ("x_proj.weight", (R + 2 * N, di)), ("dt_proj.weight", (di, R)), ("dt_proj.bias", (di,)),
                        ("A_log", (di, N)), ("D", (di,)), ("out_proj.weight", (d, di))])


def weight_floats(d, E, N, K, R):
    return sum(int(np.prod(s)) for s in weight_shapes(d, E, N, K, R).values())


def split_weights(flat, d, E, N, K, R):
    out, off = OrderedDict(), 0
    for k, shp in weight_shapes(d, E, N, K, R).items():
        n = int(np.prod(shp))
        out[k] = flat[off:off + n].reshape(shp)
        off += n
    assert off == flat.size
    return out


def flat_weights(w, d, E, N, K, R):
    return np.concatenate([np.asarray(w[k]).reshape(-1) for k in weight_shapes(d, E, N, K, R)])


def dt_rank(d):
    return 4 * math.ceil(d / 64)


def random_weights(rng, d, E, N, K, R, std=0.02):
    """fp32 flat weights with the model's init: Linear weights N(0, std), conv1d U(+-K^-1/2), dt_proj.weight U(+-R^-1/2),
    dt_proj.bias = softplus^-1(dt) with dt log-uniform in [1e-3, 1e-1], A_log[j, n] = log(n + 1), D = 1."""
    di = E * d
    dt = np.exp(rng.uniform(math.log(1e-3), math.log(1e-1), di))
    w = {"in_proj.weight": rng.normal(0, std, (2 * di, d)), "conv1d.weight": rng.uniform(-K ** -0.5, K ** -0.5, (di, K)),
         "conv1d.bias": rng.uniform(-K ** -0.5, K ** -0.5, di), "x_proj.weight": rng.normal(0, std, (R + 2 * N, di)),
         "dt_proj.weight": rng.uniform(-R ** -0.5, R ** -0.5, (di, R)), "dt_proj.bias": dt + np.log(-np.expm1(-dt)),
         "A_log": np.broadcast_to(np.log(np.arange(1, N + 1, dtype=np.float64)), (di, N)), "D": np.ones(di),
         "out_proj.weight": rng.normal(0, std, (d, di))}
    return flat_weights(w, d, E, N, K, R).astype(np.float32)


def _sig(v):
    return 0.5 * (1.0 + np.tanh(0.5 * v))                           # the logistic function, no overflow


def forward(x, ids, flat, hyper):
    """out [B, L, d] and what the backward needs.  hyper = (E, N, K, R)."""
    E, N, K, R = hyper
    B, L, d = x.shape
    di = E * d
    w = {k: v.astype(np.float64) for k, v in split_weights(np.asarray(flat), d, E, N, K, R).items()}
    x = x.astype(np.float64)
    mb = np.ones((B, L), bool) if ids is None else (ids != 0)
    m = mb.astype(np.float64)[..., None]
    xz = x @ w["in_proj.weight"].T
    xs, z = xz[..., :di], xz[..., di:]
    xm = m * xs
    c = np.broadcast_to(w["conv1d.bias"], (B, L, di)).copy()
    for k in range(K):
        back = K - 1 - k
        if back < L:
            c[:, back:] += w["conv1d.weight"][:, k] * xm[:, :L - back]
    u = c * _sig(c)
    xdbl = u @ w["x_proj.weight"].T
    delta, Bm, Cm = xdbl[..., :R], xdbl[..., R:R + N], xdbl[..., R + N:]
    dtr = delta @ w["dt_proj.weight"].T + w["dt_proj.bias"]
    dt = np.logaddexp(0.0, dtr)
    A = -np.exp(w["A_log"])
    H = np.zeros((B, L, di, N))
    h = np.zeros((B, di, N))
    for t in range(L):
        a = np.exp(dt[:, t, :, None] * A)
        hn = a * h + dt[:, t, :, None] * Bm[:, t, None, :] * u[:, t, :, None]
        h = np.where(mb[:, t, None, None], hn, h)
        H[:, t] = h
    s = (H * Cm[:, :, None, :]).sum(-1) + w["D"] * u
    y = np.where(mb[..., None], s * (z * _sig(z)), 0.0)
    out = y @ w["out_proj.weight"].T
    return out, dict(x=x, mb=mb, m=m, w=w, xs=xs, z=z, xm=xm, c=c, u=u, delta=delta, Bm=Bm, Cm=Cm, dtr=dtr, dt=dt, A=A, H=H, s=s,
                     y=y, hyper=hyper)


def backward(c, dout):
    """dx [B, L, d] and the flat weight gradient."""
    E, N, K, R = c["hyper"]
    w, mb, m, x = c["w"], c["mb"], c["m"], c["x"]
    B, L, d = x.shape
    di = E * d
    dout = dout.astype(np.float64)
    u, z, dt, A, H, Bm, Cm = c["u"], c["z"], c["dt"], c["A"], c["H"], c["Bm"], c["Cm"]
    dy = dout @ w["out_proj.weight"]
    sz = _sig(z)
    ds = np.where(mb[..., None], dy * (z * sz), 0.0)
    dz = np.where(mb[..., None], dy * c["s"] * (sz * (1.0 + z * (1.0 - sz))), 0.0)
    du = ds * w["D"]
    ddt, dB, dC = np.zeros((B, L, di)), np.zeros((B, L, N)), np.zeros((B, L, N))
    dA = np.zeros((di, N))
    carry = np.zeros((B, di, N))
    for t in range(L - 1, -1, -1):
        mt = mb[:, t, None, None]
        e = ds[:, t, :, None] * Cm[:, t, None, :] + carry
        dC[:, t] = (ds[:, t, :, None] * H[:, t]).sum(1)
        hprev = H[:, t - 1] if t > 0 else np.zeros((B, di, N))
        a = np.exp(dt[:, t, :, None] * A)
        em = np.where(mt, e, 0.0)                                      # an item's position alone feeds the step's inputs
        da = em * hprev
        ddt[:, t] = (da * a * A + em * Bm[:, t, None, :] * u[:, t, :, None]).sum(-1)
        dA += (da * a * dt[:, t, :, None]).sum(0)
        dB[:, t] = (em * dt[:, t, :, None] * u[:, t, :, None]).sum(1)
        du[:, t] += (em * dt[:, t, :, None] * Bm[:, t, None, :]).sum(-1)
        carry = np.where(mt, a * e, e)
    ddtr = ddt * _sig(c["dtr"])
    dxdbl = np.concatenate([ddtr @ w["dt_proj.weight"], dB, dC], -1)
    du = du + dxdbl @ w["x_proj.weight"]
    cc = c["c"]
    sc = _sig(cc)
    dc = du * (sc * (1.0 + cc * (1.0 - sc)))
    dwc, dxm = np.zeros((di, K)), np.zeros((B, L, di))
    for k in range(K):
        back = K - 1 - k
        if back < L:
            dwc[:, k] = (dc[:, back:] * c["xm"][:, :L - back]).sum((0, 1))
            dxm[:, :L - back] += w["conv1d.weight"][:, k] * dc[:, back:]
    dxz = np.concatenate([m * dxm, dz], -1)
    T = B * L
    r = lambda a: a.reshape(T, -1)
    dw = {"in_proj.weight": r(dxz).T @ r(x), "conv1d.weight": dwc, "conv1d.bias": dc.sum((0, 1)),
          "x_proj.weight": r(dxdbl).T @ r(u), "dt_proj.weight": r(ddtr).T @ r(c["delta"]), "dt_proj.bias": ddtr.sum((0, 1)),
          "A_log": dA * A, "D": (ds * u).sum((0, 1)), "out_proj.weight": r(dout).T @ r(c["y"])}
    return dxz @ w["in_proj.weight"], flat_weights(dw, d, E, N, K, R)


def torch_layer(x, ids, w, hyper):
    """The layer in torch ops with a Python loop over t, differentiable: ``w`` maps the nine names to tensors."""
    import torch
    import torch.nn.functional as F
    E, N, K, R = hyper
    B, L, d = x.shape
    di = E * d
    mb = torch.ones(B, L, dtype=torch.bool, device=x.device) if ids is None else (ids != 0)
    xz = x @ w["in_proj.weight"].T
    xs, z = xz[..., :di], xz[..., di:]
    xm = torch.where(mb[..., None], xs, torch.zeros_like(xs))
    xp = F.pad(xm, (0, 0, K - 1, 0))
    c = w["conv1d.bias"] + sum(w["conv1d.weight"][:, k] * xp[:, k:k + L] for k in range(K))
    u = F.silu(c)
    xdbl = u @ w["x_proj.weight"].T
    delta, Bm, Cm = xdbl[..., :R], xdbl[..., R:R + N], xdbl[..., R + N:]
    dt = F.softplus(delta @ w["dt_proj.weight"].T + w["dt_proj.bias"])
    A = -torch.exp(w["A_log"])
    h, ss = torch.zeros(B, di, N, dtype=x.dtype, device=x.device), []
    for t in range(L):
        hn = torch.exp(dt[:, t, :, None] * A) * h + dt[:, t, :, None] * Bm[:, t, None, :] * u[:, t, :, None]
        h = torch.where(mb[:, t, None, None], hn, h)
        ss.append((h * Cm[:, t, None, :]).sum(-1))
    s = torch.stack(ss, 1) + w["D"] * u
    y = torch.where(mb[..., None], s * F.silu(z), torch.zeros_like(s))
    return y @ w["out_proj.weight"].T


# ---- the whole model --------------------------------------------------------------------------------------------------------
def layer_flat(sd, k, hyper):
    """The flat weight array of block k from a state_dict-like mapping of numpy arrays."""
    E, N, K, R = hyper
    p = f"item_encoder.blocks.{k}.mamba."
    d = sd[p + "out_proj.weight"].shape[0]
    return flat_weights({n: sd[p + n] for n in weight_shapes(d, E, N, K, R)}, d, E, N, K, R)


def model_loss(sd, ids, answers, num_layers, hyper):
    """The model's loss and last-block output in numpy fp64 from a mapping name -> array (dropout 0)."""
    from scipy.special import erf
    sd = {k: np.asarray(v, dtype=np.float64) for k, v in sd.items()}
    Emb = sd["item_embeddings.weight"]
    x = _ln(np, Emb[ids], sd["LayerNorm.weight"], sd["LayerNorm.bias"], np.sqrt)
    for k in range(num_layers):
        p = f"item_encoder.blocks.{k}."
        z, _ = forward(x, ids, layer_flat(sd, k, hyper), hyper)
        a = _ln(np, z + x, sd[p + "mamba.LayerNorm.weight"], sd[p + "mamba.LayerNorm.bias"], np.sqrt)
        f = a @ sd[p + "feed_forward.dense_1.weight"].T + sd[p + "feed_forward.dense_1.bias"]
        f = f * 0.5 * (1.0 + erf(f / math.sqrt(2.0)))
        f = f @ sd[p + "feed_forward.dense_2.weight"].T + sd[p + "feed_forward.dense_2.bias"]
        x = _ln(np, f + a, sd[p + "feed_forward.LayerNorm.weight"], sd[p + "feed_forward.LayerNorm.bias"], np.sqrt)
    logits = x[:, -1] @ Emb.T
    mx = logits.max(1, keepdims=True)
    lse = np.log(np.exp(logits - mx).sum(1)) + mx[:, 0]
    return float((lse - logits[np.arange(len(answers)), answers]).mean()), x


def twin_forward(params, ids, num_layers, hyper):
    """The model in torch on the CPU, differentiable in ``params`` (name -> tensor); the recurrent layer is ``torch_layer``.
    Returns the last block's [B, L, d]."""
    import torch
    E, N, K, R = hyper
    tids = torch.as_tensor(np.asarray(ids))
    Emb = params["item_embeddings.weight"]
    d = Emb.shape[1]
    x = _ln(torch, Emb[tids], params["LayerNorm.weight"], params["LayerNorm.bias"], torch.sqrt)
    for k in range(num_layers):
        p = f"item_encoder.blocks.{k}."
        z = torch_layer(x, tids, {n: params[p + "mamba." + n] for n in weight_shapes(d, E, N, K, R)}, hyper)
        a = _ln(torch, z + x, params[p + "mamba.LayerNorm.weight"], params[p + "mamba.LayerNorm.bias"], torch.sqrt)
        f = a @ params[p + "feed_forward.dense_1.weight"].T + params[p + "feed_forward.dense_1.bias"]
        f = f * 0.5 * (1.0 + torch.erf(f / math.sqrt(2.0)))
        f = f @ params[p + "feed_forward.dense_2.weight"].T + params[p + "feed_forward.dense_2.bias"]
        x = _ln(torch, f + a, params[p + "feed_forward.LayerNorm.weight"], params[p + "feed_forward.LayerNorm.bias"], torch.sqrt)
    return x


def twin_loss(params, ids, answers, num_layers, hyper):
    import torch
    x = twin_forward(params, ids, num_layers, hyper)
    a = torch.as_tensor(np.asarray(answers), dtype=torch.int64)
    return torch.nn.functional.cross_entropy(x[:, -1] @ params["item_embeddings.weight"].T, a), x
