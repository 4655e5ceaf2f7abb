"""One LRURec training step in numpy double (bsarec_lrurec_loss_grad / bsarec_lrurec_train_step, include/bsarec_hip.h): lookup,
LayerNorm, the blocks (the recurrent layer is lru_ref's), the cross-entropy of position L - 1 over the whole catalogue, every
gradient (the item table's as the head's dense part plus np.add.at over the tokens) and Adam in the arithmetic of
oracle.bsarec_oracle.adam_step.  Dropout comes in as EXPLICIT multipliers, one [B, L, d] array per site (keep / (1 - p)): site 0
on the embeddings, 1 + 2 k behind block k's recurrent layer, 2 + 2 k behind its dense_2.  Parameters travel as {state_dict key:
float64 array} in the state_dict's order.

The recurrent layer enters the step as a ``Layer`` description (as LrrLayer does in the host driver), so that this module is also
the step of every other block model: mamba4rec_step_ref passes the state-space layer's description and keeps nothing else."""
import collections
import math

import numpy as np
from scipy.special import erf

import lru_ref as R
from oracle import bsarec_oracle as O

LN_EPS = 1e-12

# prefix: the layer's name in the state_dict keys; forward(x, ids, P, k) -> (z, cache) with block k's weights taken from P;
# backward(cache, dz, d) -> (dx, {name: gradient}); keys(N, d): the state_dict keys of the whole model, in order
Layer = collections.namedtuple("Layer", "prefix forward backward keys")


def keys(N, d=4):
    """The state_dict keys of LRURecModel, in order."""
    out = ["item_embeddings.weight", "LayerNorm.weight", "LayerNorm.bias"]
    for k in range(N):
        p = f"item_encoder.blocks.{k}."
        out += [p + "lru." + n for n in R.weight_shapes(d)] + [p + "lru.LayerNorm.weight", p + "lru.LayerNorm.bias"]
        out += [p + f"feed_forward.{m}.{w}" for m in ("dense_1", "dense_2", "LayerNorm") for w in ("weight", "bias")]
    return out


def dropout_mults(B, L, d, N, p, seed, step):
    """The 1 + 2 N multipliers of the library's Philox stream at step counter ``step``: site s, element (b L + t) d + c."""
    if p <= 0.0:
        return [np.ones((B, L, d)) for _ in range(1 + 2 * N)]
    return [O.dropout_keep(B * L * d, p, int(seed), int(step), s).reshape(B, L, d).astype(np.float64) / (1.0 - p)
            for s in range(1 + 2 * N)]


def _ln_fwd(x, w, b):
    xc = x - x.mean(-1, keepdims=True)
    rstd = 1.0 / np.sqrt((xc * xc).mean(-1, keepdims=True) + LN_EPS)
    xhat = xc * rstd
    return w * xhat + b, (xhat, rstd, w)


def _ln_bwd(cache, dy):
    xhat, rstd, w = cache
    g = dy * w
    dx = rstd * (g - g.mean(-1, keepdims=True) - xhat * (g * xhat).mean(-1, keepdims=True))
    return dx, (dy * xhat).reshape(-1, xhat.shape[-1]).sum(0), dy.reshape(-1, xhat.shape[-1]).sum(0)


def _gelu(u):
    return u * 0.5 * (1.0 + erf(u / math.sqrt(2.0)))


def _gelu_grad(u):
    return 0.5 * (1.0 + erf(u / math.sqrt(2.0))) + u * np.exp(-0.5 * u * u) / math.sqrt(2.0 * math.pi)


def _lru_backward(cache, dz, d):
    dx, dflat = R.backward(cache, dz)
    return dx, R.split_weights(dflat, d)


LRU = Layer("lru", lambda x, ids, P, k: R.forward(x, ids, R.layer_flat(P, k)), _lru_backward, keys)


def loss_and_grads(params, ids, answers, N, mults=None, layer=LRU):
    """-> (loss, {key: gradient}, x_N [B, L, d]).  ``mults``: the 1 + 2 N dropout multipliers (None: no dropout)."""
    lp = layer.prefix
    P = {k: np.asarray(v, np.float64) for k, v in params.items()}
    E = P["item_embeddings.weight"]
    ids, answers = np.asarray(ids, np.int64), np.asarray(answers, np.int64)
    B, L = ids.shape
    V, d = E.shape
    T = B * L
    mults = [np.ones((B, L, d))] * (1 + 2 * N) if mults is None else [np.asarray(m, np.float64) for m in mults]
    assert len(mults) == 1 + 2 * N
    n0, ln0 = _ln_fwd(E[ids], P["LayerNorm.weight"], P["LayerNorm.bias"])
    x = n0 * mults[0]
    blocks = []
    for k in range(N):
        p = f"item_encoder.blocks.{k}."
        z, cache = layer.forward(x, ids, P, k)
        a, ln_a = _ln_fwd(z * mults[1 + 2 * k] + x, P[p + lp + ".LayerNorm.weight"], P[p + lp + ".LayerNorm.bias"])
        u = a @ P[p + "feed_forward.dense_1.weight"].T + P[p + "feed_forward.dense_1.bias"]
        g = _gelu(u)
        f = g @ P[p + "feed_forward.dense_2.weight"].T + P[p + "feed_forward.dense_2.bias"]
        x, ln_f = _ln_fwd(f * mults[2 + 2 * k] + a, P[p + "feed_forward.LayerNorm.weight"], P[p + "feed_forward.LayerNorm.bias"])
        blocks.append((cache, ln_a, a, u, g, ln_f))
    out = x
    h = x[:, L - 1]
    logits = h @ E.T
    mx = logits.max(1, keepdims=True)
    ex = np.exp(logits - mx)
    lse = np.log(ex.sum(1)) + mx[:, 0]
    loss = float((lse - logits[np.arange(B), answers]).mean())
    # ---- backward
    dl = ex / ex.sum(1, keepdims=True)
    dl[np.arange(B), answers] -= 1.0
    dl /= B
    grads = {"item_embeddings.weight": dl.T @ h}
    dx = np.zeros((B, L, d))
    dx[:, L - 1] = dl @ E
    for k in range(N - 1, -1, -1):
        p = f"item_encoder.blocks.{k}."
        cache, ln_a, a, u, g, ln_f = blocks[k]
        ds2, grads[p + "feed_forward.LayerNorm.weight"], grads[p + "feed_forward.LayerNorm.bias"] = _ln_bwd(ln_f, dx)
        df = (ds2 * mults[2 + 2 * k]).reshape(T, d)
        grads[p + "feed_forward.dense_2.weight"], grads[p + "feed_forward.dense_2.bias"] = df.T @ g.reshape(T, 4 * d), df.sum(0)
        du = (df @ P[p + "feed_forward.dense_2.weight"]) * _gelu_grad(u.reshape(T, 4 * d))
        grads[p + "feed_forward.dense_1.weight"], grads[p + "feed_forward.dense_1.bias"] = du.T @ a.reshape(T, d), du.sum(0)
        da = ds2 + (du @ P[p + "feed_forward.dense_1.weight"]).reshape(B, L, d)
        ds1, grads[p + lp + ".LayerNorm.weight"], grads[p + lp + ".LayerNorm.bias"] = _ln_bwd(ln_a, da)
        dxl, dw = layer.backward(cache, ds1 * mults[1 + 2 * k], d)
        for n, v in dw.items():
            grads[p + lp + "." + n] = np.ascontiguousarray(v)
        dx = dxl + ds1
    de, grads["LayerNorm.weight"], grads["LayerNorm.bias"] = _ln_bwd(ln0, dx * mults[0])
    np.add.at(grads["item_embeddings.weight"], ids.reshape(-1), de.reshape(T, d))
    return loss, {k: grads[k] for k in layer.keys(N, d)}, out


def adam_state(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    return O.AdamState(lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay)


def train_step(params, st, ids, answers, N, mults=None, layer=LRU):
    """One step in place: the gradients at ``params``, then oracle.adam_step.  Returns the loss."""
    loss, grads, _ = loss_and_grads(params, ids, answers, N, mults, layer)
    O.adam_step(params, grads, st)
    return loss
