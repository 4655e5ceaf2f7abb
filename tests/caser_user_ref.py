"""One step of the personalised Caser (args.caser_user) in numpy double, on the parts of caser_ref / caser_step_ref:
  x = E[ids];  z = CaserConv(x);  z1 = relu(fc1(z (.) mult));  x2 = [z1 | P[users]];  s = relu(fc2(x2));  BPR on s
with every gradient and Adam in the arithmetic of oracle.bsarec_oracle.adam_step.  A user id outside [0, U) is no row: its half of
x2 is zero and it adds nothing to dP.  Parameters travel as {state_dict key: float64 array} in the state_dict's order."""
import numpy as np

import caser_ref as R
import caser_step_ref as S
from oracle import bsarec_oracle as O

adam_state = S.adam_state
dropout_mult = S.dropout_mult


def keys(L):
    """The state_dict keys of CaserModel with caser_user, in order."""
    k = S.keys(L)
    return k[:1] + ["user_embeddings.weight"] + k[1:] + ["fc2.weight", "fc2.bias"]


def forward(params, ids, users, mult=None):
    """-> dict(z, cache, zd, u1, z1, inside, x2, u2, s): every stage of the forward, u1 / u2 the pre-activations of fc1 / fc2."""
    L, d, nh, nv = S.shape_of(params)
    E, P = (np.asarray(params[k], np.float64) for k in ("item_embeddings.weight", "user_embeddings.weight"))
    ids, users = np.asarray(ids, np.int64), np.asarray(users, np.int64).reshape(-1)
    z, cache = R.forward(E[ids], S.flat_of(params), nh, nv)
    zd = z if mult is None else z * mult
    u1 = zd @ np.asarray(params["fc1.weight"], np.float64).T + np.asarray(params["fc1.bias"], np.float64)
    z1 = np.maximum(u1, 0.0)
    inside = (users >= 0) & (users < P.shape[0])
    pu = P[np.clip(users, 0, P.shape[0] - 1)] * inside[:, None]
    x2 = np.concatenate([z1, pu], 1)
    u2 = x2 @ np.asarray(params["fc2.weight"], np.float64).T + np.asarray(params["fc2.bias"], np.float64)
    return dict(z=z, cache=cache, zd=zd, u1=u1, z1=z1, inside=inside, x2=x2, u2=u2, s=np.maximum(u2, 0.0))


def condition(params, ids, users, mult=None, margin=1e-4):
    """(number of ambiguous convolution cells, min |u| over the pre-activations of fc1 AND fc2) at these weights: the discrete
    choices that fp32 cannot be asked to reproduce (caser_step_ref.condition, with fc2's ReLU beside fc1's)."""
    f = forward(params, ids, users, mult)
    return int(R.ambiguous(f["cache"], margin).sum()), float(min(np.abs(f["u1"]).min(), np.abs(f["u2"]).min()))


def loss_and_grads(params, ids, users, pos, neg, mult=None):
    """-> (loss, dict(z1, x2, s), {key: gradient}).  ``mult`` [B, F] multiplies z (None: no dropout)."""
    L, d, nh, nv = S.shape_of(params)
    ids, pos, neg = (np.asarray(v, np.int64) for v in (ids, pos, neg))
    users = np.asarray(users, np.int64).reshape(-1)
    E = np.asarray(params["item_embeddings.weight"], np.float64)
    W1, W2 = (np.asarray(params[k], np.float64) for k in ("fc1.weight", "fc2.weight"))
    f = forward(params, ids, users, mult)
    loss, ds, dpos, dneg = R.bpr(f["s"], E[pos], E[neg])
    du2 = ds * (f["u2"] > 0)
    dx2 = du2 @ W2
    dP = np.zeros_like(np.asarray(params["user_embeddings.weight"], np.float64))
    np.add.at(dP, users[f["inside"]], dx2[f["inside"], d:])
    du1 = dx2[:, :d] * (f["u1"] > 0)
    dzd = du1 @ W1
    dx, dflat = R.backward(f["cache"], dzd if mult is None else dzd * mult)
    dE = np.zeros_like(E)
    np.add.at(dE, ids.reshape(-1), dx.reshape(-1, d))
    np.add.at(dE, pos, dpos)
    np.add.at(dE, neg, dneg)
    grads = {"item_embeddings.weight": dE, "user_embeddings.weight": dP, "fc1.weight": du1.T @ f["zd"], "fc1.bias": du1.sum(0),
             "fc2.weight": du2.T @ f["x2"], "fc2.bias": du2.sum(0)}
    for name, w in R.split_weights(dflat, L, d, nh, nv).items():
        grads["conv." + name] = w.reshape(params["conv." + name].shape)
    return loss, {k: f[k] for k in ("z1", "x2", "s")}, {k: grads[k] for k in keys(L)}


def train_step(params, st, ids, users, pos, neg, mult=None):
    """One step in place: the gradients at ``params``, then oracle.adam_step.  Returns the loss."""
    loss, _, grads = loss_and_grads(params, ids, users, pos, neg, mult)
    O.adam_step(params, grads, st)
    return loss
