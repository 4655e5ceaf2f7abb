"""One Caser training step in numpy double: gather, convolution block, the Philox mask on z, fc1 + ReLU, BPR head, every gradient
(caser_ref.model_loss_grads) and Adam in the arithmetic of oracle.bsarec_oracle.adam_step.  Parameters travel as
{state_dict key: float64 array} in the state_dict's order and with its (Conv2d) shapes."""
import numpy as np

import caser_ref as R
from oracle import bsarec_oracle as O


def keys(L):
    """The state_dict keys of CaserModel, in order."""
    out = ["item_embeddings.weight", "conv.conv_v.weight", "conv.conv_v.bias"]
    for i in range(L):
        out += [f"conv.conv_h.{i}.weight", f"conv.conv_h.{i}.bias"]
    return out + ["fc1.weight", "fc1.bias"]


def shape_of(params, nh=None):
    """(L, d, n_h, n_v) of a parameter dictionary."""
    nv, _, L, _ = params["conv.conv_v.weight"].shape
    return L, params["item_embeddings.weight"].shape[1], params["conv.conv_h.0.weight"].shape[0], nv


def flat_of(params):
    """The convolution's parameters as the padded flat array of bsarec_caser_fwd."""
    L, d, nh, nv = shape_of(params)
    return R.flat_weights({k[5:]: v for k, v in params.items() if k.startswith("conv.")}, L, d, nh, nv)


def dropout_mult(B, F, p, seed, step):
    """Keep-mask times 1 / (1 - p) of dropout site 0 at step counter ``step``, [B, F]: element b F + k of the stream."""
    if p <= 0.0:
        return np.ones((B, F))
    return O.dropout_keep(B * F, p, int(seed), int(step), 0).reshape(B, F).astype(np.float64) / (1.0 - p)


def condition(params, ids, mult=None, margin=1e-4):
    """(number of ambiguous convolution cells, min |u|) at these weights: what fp32 cannot be asked to reproduce -- a cell whose
    ReLU switch or argmax is decided within ``margin`` (caser_ref.ambiguous), a pre-activation of fc1 that close to 0."""
    L, d, nh, nv = shape_of(params)
    E = np.asarray(params["item_embeddings.weight"], np.float64)
    z, cache = R.forward(E[np.asarray(ids)], flat_of(params), nh, nv)
    zd = z if mult is None else z * mult
    u = zd @ np.asarray(params["fc1.weight"], np.float64).T + np.asarray(params["fc1.bias"], np.float64)
    return int(R.ambiguous(cache, margin).sum()), float(np.abs(u).min())


def loss_and_grads(params, ids, pos, neg, mult=None):
    """-> (loss, s, {key: gradient}).  ``mult`` [B, F] multiplies z (None: no dropout)."""
    L, d, nh, nv = shape_of(params)
    ids, pos, neg = (np.asarray(v, np.int64) for v in (ids, pos, neg))
    loss, s, g = R.model_loss_grads(params["item_embeddings.weight"], flat_of(params), params["fc1.weight"], params["fc1.bias"],
                                    ids, pos, neg, nh, nv, mult, 0.0)
    grads = {k: g[k] for k in ("item_embeddings.weight", "fc1.weight", "fc1.bias")}
    for name, w in R.split_weights(g["conv"], L, d, nh, nv).items():
        grads["conv." + name] = w.reshape(params["conv." + name].shape)
    return loss, s, {k: grads[k] for k in keys(L)}


def adam_state(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    return O.AdamState(lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay)


def train_step(params, st, ids, pos, neg, mult=None):
    """One step in place: the gradients at ``params``, then oracle.adam_step.  Returns the loss."""
    loss, _, grads = loss_and_grads(params, ids, pos, neg, mult)
    O.adam_step(params, grads, st)
    return loss
