"""One Mamba4Rec training step in numpy double (bsarec_mamba4rec_loss_grad / bsarec_mamba4rec_train_step, include/bsarec_hip.h):
lrurec_step_ref's step with the selective state-space layer of mamba_ref inside a block, given to it as a ``Layer`` description.
This module keeps what is Mamba4Rec's own: the state_dict keys, the order of the step's flat weight array, and the layer.
Dropout multipliers and parameters travel as in lrurec_step_ref; ``hyper`` is the layer's (expand, d_state, d_conv, dt_rank)."""
import mamba_ref as M
import lrurec_step_ref as B
from lrurec_step_ref import adam_state, dropout_mults  # noqa: F401


def _keys(N, names):
    out = ["LayerNorm.weight", "LayerNorm.bias"]
    for k in range(N):
        p = f"item_encoder.blocks.{k}."
        out += [p + "mamba." + n for n in names] + [p + "mamba.LayerNorm.weight", p + "mamba.LayerNorm.bias"]
        out += [p + f"feed_forward.{m}.{w}" for m in ("dense_1", "dense_2", "LayerNorm") for w in ("weight", "bias")]
    return out


def keys(N, hyper, d=4):
    """The state_dict keys of Mamba4RecModel, in order: a layer's own parameters (A_log, D) stand before those of its children,
    so the order inside a layer is not the flat weight array's (``flat_keys``)."""
    own = ["A_log", "D"]
    return ["item_embeddings.weight"] + _keys(N, own + [n for n in M.weight_shapes(d, *hyper) if n not in own])


def flat_keys(N, hyper, d=4):
    """The keys of every tensor but the item table in the order of the step's flat weight array: a layer's tensors in the order
    of bsarec_mamba_fwd's array."""
    return _keys(N, list(M.weight_shapes(d, *hyper)))


def layer(hyper):
    """The state-space layer as lrurec_step_ref takes it."""
    def backward(cache, dz, d):
        dx, dflat = M.backward(cache, dz)
        return dx, M.split_weights(dflat, d, *hyper)
    return B.Layer("mamba", lambda x, ids, P, k: M.forward(x, ids, M.layer_flat(P, k, hyper), hyper), backward,
                   lambda N, d: keys(N, hyper, d))


def loss_and_grads(params, ids, answers, N, hyper, mults=None):
    """-> (loss, {key: gradient}, x_N [B, L, d]).  ``mults``: the 1 + 2 N dropout multipliers (None: no dropout)."""
    return B.loss_and_grads(params, ids, answers, N, mults, layer(hyper))


def train_step(params, st, ids, answers, N, hyper, mults=None):
    """One step in place: the gradients at ``params``, then oracle.adam_step.  Returns the loss."""
    return B.train_step(params, st, ids, answers, N, mults, layer(hyper))
