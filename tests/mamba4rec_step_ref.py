"""One Mamba4Rec training step in numpy double (bsarec_mamba4rec_loss_grad / bsarec_mamba4rec_train_step, include/bsarec_hip.h):
lrurec_step_ref's step with the selective state-space layer of mamba_ref inside a block -- lookup, LayerNorm, the blocks, the
cross-entropy of position L - 1 over the whole catalogue, every gradient (the item table's as the head's dense part plus
np.add.at over the tokens) and Adam in the arithmetic of oracle.bsarec_oracle.adam_step.  Dropout comes in as EXPLICIT
multipliers, one [B, L, d] array per site (keep / (1 - p)): site 0 on the embeddings, 1 + 2 k behind block k's state-space layer,
2 + 2 k behind its dense_2.  Parameters travel as {state_dict key: float64 array} in the state_dict's order; ``hyper`` is the
layer's (expand, d_state, d_conv, dt_rank)."""
import numpy as np

import mamba_ref as M
from lrurec_step_ref import _gelu, _gelu_grad, _ln_bwd, _ln_fwd, adam_state, dropout_mults  # noqa: F401
from oracle import bsarec_oracle as O


def keys(N, hyper, d=4):
    """The state_dict keys of Mamba4RecModel, in order: a layer's own parameters (A_log, D) stand before those of its children,
    so the order inside a layer is not the flat weight array's (``flat_keys``)."""
    out = ["item_embeddings.weight", "LayerNorm.weight", "LayerNorm.bias"]
    for k in range(N):
        p = f"item_encoder.blocks.{k}."
        names = list(M.weight_shapes(d, *hyper))
        out += [p + "mamba." + n for n in ["A_log", "D"] + [n for n in names if n not in ("A_log", "D")]]
        out += [p + "mamba.LayerNorm.weight", p + "mamba.LayerNorm.bias"]
        out += [p + f"feed_forward.{m}.{w}" for m in ("dense_1", "dense_2", "LayerNorm") for w in ("weight", "bias")]
    return out


def flat_keys(N, hyper, d=4):
    """The keys of every tensor but the item table in the order of the step's flat weight array: a layer's tensors in the order
    of bsarec_mamba_fwd's array."""
    out = ["LayerNorm.weight", "LayerNorm.bias"]
    for k in range(N):
        p = f"item_encoder.blocks.{k}."
        out += [p + "mamba." + n for n in M.weight_shapes(d, *hyper)] + [p + "mamba.LayerNorm.weight", p + "mamba.LayerNorm.bias"]
        out += [p + f"feed_forward.{m}.{w}" for m in ("dense_1", "dense_2", "LayerNorm") for w in ("weight", "bias")]
    return out


def loss_and_grads(params, ids, answers, N, hyper, mults=None):
    """-> (loss, {key: gradient}, x_N [B, L, d]).  ``mults``: the 1 + 2 N dropout multipliers (None: no dropout)."""
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
        z, layer = M.forward(x, ids, M.layer_flat(P, k, hyper), hyper)
        a, ln_a = _ln_fwd(z * mults[1 + 2 * k] + x, P[p + "mamba.LayerNorm.weight"], P[p + "mamba.LayerNorm.bias"])
        u = a @ P[p + "feed_forward.dense_1.weight"].T + P[p + "feed_forward.dense_1.bias"]
        g = _gelu(u)
        f = g @ P[p + "feed_forward.dense_2.weight"].T + P[p + "feed_forward.dense_2.bias"]
        x, ln_f = _ln_fwd(f * mults[2 + 2 * k] + a, P[p + "feed_forward.LayerNorm.weight"], P[p + "feed_forward.LayerNorm.bias"])
        blocks.append((layer, ln_a, a, u, g, ln_f))
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
        layer, ln_a, a, u, g, ln_f = blocks[k]
        ds2, grads[p + "feed_forward.LayerNorm.weight"], grads[p + "feed_forward.LayerNorm.bias"] = _ln_bwd(ln_f, dx)
        df = (ds2 * mults[2 + 2 * k]).reshape(T, d)
        grads[p + "feed_forward.dense_2.weight"], grads[p + "feed_forward.dense_2.bias"] = df.T @ g.reshape(T, 4 * d), df.sum(0)
        du = (df @ P[p + "feed_forward.dense_2.weight"]) * _gelu_grad(u.reshape(T, 4 * d))
        grads[p + "feed_forward.dense_1.weight"], grads[p + "feed_forward.dense_1.bias"] = du.T @ a.reshape(T, d), du.sum(0)
        da = ds2 + (du @ P[p + "feed_forward.dense_1.weight"]).reshape(B, L, d)
        ds1, grads[p + "mamba.LayerNorm.weight"], grads[p + "mamba.LayerNorm.bias"] = _ln_bwd(ln_a, da)
        dxl, dflat = M.backward(layer, ds1 * mults[1 + 2 * k])
        for n, v in M.split_weights(dflat, d, *hyper).items():
            grads[p + "mamba." + n] = np.ascontiguousarray(v)
        dx = dxl + ds1
    de, grads["LayerNorm.weight"], grads["LayerNorm.bias"] = _ln_bwd(ln0, dx * mults[0])
    np.add.at(grads["item_embeddings.weight"], ids.reshape(-1), de.reshape(T, d))
    return loss, {k: grads[k] for k in keys(N, hyper, d)}, out


def train_step(params, st, ids, answers, N, hyper, mults=None):
    """One step in place: the gradients at ``params``, then oracle.adam_step.  Returns the loss."""
    loss, grads, _ = loss_and_grads(params, ids, answers, N, hyper, mults)
    O.adam_step(params, grads, st)
    return loss
