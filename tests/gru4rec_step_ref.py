"""One GRU4Rec training step in numpy double: gather, dropout mask, GRU stack and projection (gru_ref), BPR head, every gradient
(the item table's with np.add.at over the tokens plus the head's two rows per sequence) and Adam in the arithmetic of
oracle.bsarec_oracle.adam_step.  Parameters travel as {state_dict key: float64 array} in the state_dict's order."""
import numpy as np

import gru_ref as R
from oracle import bsarec_oracle as O

GRU_NAMES = {"out_weight": "dense.weight", "out_bias": "dense.bias"}


def keys(N):
    """The state_dict keys of GRU4RecModel, in order."""
    out = ["item_embeddings.weight"]
    for k in range(N):
        out += [f"gru_layers.weight_ih_l{k}", f"gru_layers.weight_hh_l{k}"]
    return out + ["dense.weight", "dense.bias"]


def flat_of(params, N):
    return np.concatenate([np.asarray(params[k], np.float64).reshape(-1) for k in keys(N)[1:]])


def dropout_mult(B, L, d, p, seed, step):
    """Keep-mask times 1 / (1 - p) of dropout site 0 at step counter ``step``, [B, L, d]: element (b L + t) d + c of the stream."""
    if p <= 0.0:
        return np.ones((B, L, d))
    keep = O.dropout_keep(B * L * d, p, int(seed), int(step), 0).reshape(B, L, d)
    return keep.astype(np.float64) / (1.0 - p)


def loss_and_grads(params, ids, pos, neg, H, N, mult=None):
    """-> (loss, {key: gradient}).  ``mult`` [B, L, d] multiplies the looked-up embeddings (None: no dropout)."""
    E = np.asarray(params["item_embeddings.weight"], np.float64)
    ids, pos, neg = (np.asarray(v, np.int64) for v in (ids, pos, neg))
    B, L = ids.shape
    d = E.shape[1]
    mult = np.ones((B, L, d)) if mult is None else np.asarray(mult, np.float64)
    out, cache = R.forward(E[ids] * mult, flat_of(params, N), H, N, d)
    loss, ds, dpos, dneg = R.bpr(out[:, L - 1], E[pos], E[neg])
    dx, dflat = R.backward(cache, R.last_only_dout(ds, L))
    dE = np.zeros_like(E)
    np.add.at(dE, ids.reshape(-1), (dx * mult).reshape(-1, d))
    np.add.at(dE, pos, dpos)
    np.add.at(dE, neg, dneg)
    grads = {"item_embeddings.weight": dE}
    for name, g in R.split_weights(dflat, d, H, N, d).items():
        grads[GRU_NAMES.get(name, "gru_layers." + name)] = g
    return loss, {k: grads[k] for k in keys(N)}


def adam_state(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0):
    return O.AdamState(lr=lr, beta1=beta1, beta2=beta2, eps=eps, weight_decay=weight_decay)


def train_step(params, st, ids, pos, neg, H, N, mult=None):
    """One step in place: the gradients at ``params``, then oracle.adam_step.  Returns the loss."""
    loss, grads = loss_and_grads(params, ids, pos, neg, H, N, mult)
    O.adam_step(params, grads, st)
    return loss
