"""LRURec sibling model: an item embedding and a stack of blocks, each a linear recurrent unit (a complex diagonal linear
recurrence over the sequence) and a position-wise feed-forward net, trained with the full-catalogue cross-entropy of the last
position.

The contract of this model is the math of its docstrings, checked against an fp64 restatement (tests/lru_ref.py,
tests/test_lru_cpu.py) that is itself checked against torch's complex autograd; it was written from the LRURec paper (Yue et al.,
"Linear Recurrent Units for Sequential Recommendation", WSDM 2024) without the reference source at hand, and no reference golden
exists for it.  Where it departs from the paper's code, on purpose: the loss is taken at the last position only (the dataset
already expands every prefix), there is no item bias, and the out-projection is a real matrix on the stacked real and imaginary
parts of the state (``Re(C h)`` with the sign of the imaginary half absorbed into the parameter).  The recurrent layer runs in
libbsarec_hip.so in both directions (bsarec_lru_fwd / bsarec_lru_bwd, csrc/lru.h) and the loss in the catalogue CE head
(bsarec_ce_head_fwd / _bwd); on the default path the embedding lookup, the LayerNorms, the feed-forward net and the dropout are
torch ops.  With ``lru_step = "fused"`` the whole training step -- those parts, the item-table gradient and Adam included -- is one
C call (bsarec_lrurec_train_step, csrc/lrurec_step.h).  There is no CPU path.  The layer's and the model's plumbing, the
fused mode's included, is the siblings' shared shell (_sibling.py).
"""
from __future__ import annotations

import math
from collections import OrderedDict

import torch

from . import _lib as L
from ._sibling import _BlockModel, _FeedForward, _FlatLayer, _Holder, _LayerNorm, _act, _layout  # noqa: F401


def lru_param_shapes(width: int) -> "OrderedDict[str, tuple]":
    """The tensors of bsarec_lru_fwd's flat weight array, in its order (include/bsarec_hip.h)."""
    d = int(width)
    return OrderedDict([("nu_log", (d,)), ("theta_log", (d,)), ("gamma_log", (d,)), ("in_proj.weight", (2 * d, d)),
                        ("in_proj.bias", (2 * d,)), ("out_proj.weight", (d, 2 * d)), ("out_proj.bias", (d,))])


def lrurec_param_shapes(width: int, layers: int) -> "OrderedDict[str, tuple]":
    """The tensors of bsarec_lrurec_loss_grad's flat weight array under their state_dict keys, in its order (include/bsarec_hip.h):
    every parameter of LRURecModel but the item table."""
    d = int(width)
    shapes = OrderedDict([("LayerNorm.weight", (d,)), ("LayerNorm.bias", (d,))])
    for k in range(int(layers)):
        blk = f"item_encoder.blocks.{k}."
        for name, shp in lru_param_shapes(d).items():
            shapes[blk + "lru." + name] = shp
        shapes[blk + "lru.LayerNorm.weight"] = shapes[blk + "lru.LayerNorm.bias"] = (d,)
        shapes[blk + "feed_forward.dense_1.weight"], shapes[blk + "feed_forward.dense_1.bias"] = (4 * d, d), (4 * d,)
        shapes[blk + "feed_forward.dense_2.weight"], shapes[blk + "feed_forward.dense_2.bias"] = (d, 4 * d), (d,)
        shapes[blk + "feed_forward.LayerNorm.weight"] = shapes[blk + "feed_forward.LayerNorm.bias"] = (d,)
    return shapes


class LruLayer(_FlatLayer):
    """x [B, L, d], ids [B, L] (0 is padding; ``None``: no padding) -> y [B, L, d] on the HIP kernels, with m_t = (ids_t != 0):
      lambda = exp(-exp(nu_log)) (cos(exp(theta_log)) + i sin(exp(theta_log)))                       |lambda| < 1 always
      u_t = in_proj(x_t) (first d entries real, last d imaginary);  v_t = m_t exp(gamma_log) u_t
      h_t = lambda h_{t-1} + v_t, h_{-1} = 0;   y_t = out_proj([Re h_t | Im h_t])
    Owns ONE flat fp32 tensor in the layout of bsarec_lru_fwd's ``weights``; ``nu_log``, ``theta_log``, ``gamma_log``,
    ``in_proj.{weight,bias}`` and ``out_proj.{weight,bias}`` are parameters that are views of it, so an optimiser that updates them
    in place updates the array the kernels read.  The workspace carries v and h to the backward.

    Init: u1, u2 ~ U(0, 1) per channel, nu_log = log(-1/2 log(u1 (r_max^2 - r_min^2) + r_min^2)), theta_log = log(2 pi u2),
    gamma_log = log sqrt(1 - |lambda|^2), which puts |lambda| in [r_min, r_max]; projection weights N(0, ``std``), biases 0."""

    _tag = "lru"

    def __init__(self, width: int, r_min: float = 0.8, r_max: float = 0.99, std: float = 0.02):
        super().__init__()
        d = int(width)
        if not (4 <= d <= 256 and d % 4 == 0):
            raise ValueError(f"LRURec: hidden_size {d} outside 4..256 or not a multiple of 4")
        if not 0.0 <= r_min < r_max < 1.0:
            raise ValueError(f"LRURec: lru_r_min = {r_min}, lru_r_max = {r_max}: expected 0 <= r_min < r_max < 1")
        self.width, self.r_min, self.r_max = d, float(r_min), float(r_max)
        v = self._make_flat(lru_param_shapes(d))
        for name in ("nu_log", "theta_log", "gamma_log"):
            self.register_parameter(name, v[name])
        self.in_proj = _Holder(v["in_proj.weight"], v["in_proj.bias"])
        self.out_proj = _Holder(v["out_proj.weight"], v["out_proj.bias"])
        with torch.no_grad():
            u1, u2 = torch.rand(d, dtype=torch.float64), torch.rand(d, dtype=torch.float64)
            nu_log = torch.log(-0.5 * torch.log(u1 * (r_max ** 2 - r_min ** 2) + r_min ** 2))
            mod2 = torch.exp(-2.0 * torch.exp(nu_log))
            v["nu_log"].copy_(nu_log)
            v["theta_log"].copy_(torch.log(2.0 * math.pi * u2))
            v["gamma_log"].copy_(0.5 * torch.log(1.0 - mod2))
            v["in_proj.weight"].normal_(0.0, std)
            v["out_proj.weight"].normal_(0.0, std)

    def extra_repr(self):
        return f"width={self.width}, r_min={self.r_min}, r_max={self.r_max}"

    def _config(self, inputs, ids, train):
        x = self._scan_input(inputs, ids)
        cfg = L.LruConfig(x.shape[0], x.shape[1], self.width)
        nbytes = L.load().bsarec_lru_workspace_bytes(cfg, int(train))
        if nbytes < 0:
            raise ValueError(f"lru: unsupported shape B = {x.shape[0]}, L = {x.shape[1]} (1 <= B <= 65536, 1 <= L <= 256)")
        return cfg, nbytes

    def _fwd(self, cfg, inputs, ids, train, y, ws, nbytes, stream):
        L.check(L.load().bsarec_lru_fwd(cfg, inputs[0].data_ptr(), None if ids is None else ids.data_ptr(), self._flat.data_ptr(),
                                        train, y.data_ptr(), ws.data_ptr(), nbytes, stream), "bsarec_lru_fwd")

    def _bwd(self, cfg, inputs, ids, flat, g, ws, nbytes, grads, dw, stream):
        L.check(L.load().bsarec_lru_bwd(cfg, inputs[0].data_ptr(), None if ids is None else ids.data_ptr(), flat.data_ptr(),
                                        g.data_ptr(), ws.data_ptr(), nbytes, grads[0].data_ptr(), dw.data_ptr(), stream),
                "bsarec_lru_bwd")

    def forward(self, x, ids=None):
        """Differentiable with respect to x and every parameter when autograd is recording; otherwise the train = 0 call,
        which keeps nothing."""
        return self._call((x,), None if ids is None else ids.to(torch.int64).contiguous())


class LRURecModel(_BlockModel):
    """``bsarec_amd.main.MODEL_REGISTRY['lrurec']`` (``--model_type LRURec``).  State_dict keys: ``item_embeddings.weight``
    [V, d], ``LayerNorm.{weight,bias}``, and per block k < N = num_hidden_layers ``item_encoder.blocks.{k}.lru.{nu_log,theta_log,
    gamma_log}`` [d], ``...lru.in_proj.{weight,bias}`` [2d, d] / [2d], ``...lru.out_proj.{weight,bias}`` [d, 2d] / [d],
    ``...lru.LayerNorm.{weight,bias}``, ``...feed_forward.{dense_1,dense_2,LayerNorm}.{weight,bias}`` (4d inner).

    forward: x = Dropout(LN(E[ids])) -- no position embedding, the recurrence carries the order; per block k:
      z = LruLayer_k(x, ids);  a = LN(Dropout(z) + x);  x = LN(Dropout(dense_2(gelu(dense_1(a)))) + a)
    LayerNorm is TF style with eps 1e-12, gelu the erf form, every dropout ``hidden_dropout_prob`` with draws from a torch
    generator seeded by ``set_seed``.  Sequences are left-padded with id 0; padded inputs are masked inside the layer, so the
    state is 0 until a sequence's first item.
    Loss: ``cross_entropy(x[:, L - 1] @ E.T, answers)`` as one HIP node (no [B, V] logits).
    Init: Embedding and Linear weights N(0, initializer_range), biases 0, LayerNorm 1 / 0, the recurrent parameters as
    ``LruLayer`` has them with ``lru_r_min`` (default 0.8) and ``lru_r_max`` (default 0.99).

    ``args.lru_step`` selects how the model steps, single GPU either way:
      "torch" (the default, also when absent): calculate_loss / backward / torch.optim.Adam (``torch_optim``); the dropout masks
        are drawn from a torch generator seeded by ``set_seed``.
      "fused": ``train_step`` is ONE C call (bsarec_lrurec_train_step: lookup, every LayerNorm, the recurrent layers, the
        feed-forward nets, the CE head, every gradient, Adam on the item table and on the flat weight array), replayed from a
        hipGraph per batch shape unless ``args.lru_step_graph`` is False.  The model then owns ONE flat fp32 tensor in the layout
        of bsarec_lrurec_loss_grad's ``weights`` (``lrurec_param_shapes``); every parameter but the item table is a view of it and
        each ``LruLayer._flat`` a slice of it, so state_dict keys and shapes are those of the default mode and checkpoints pass
        between the two.  The instance sets ``torch_optim = False`` and ``own_train_step = True``, which is what Trainer.iteration
        routes by.  Its dropout masks are the library's Philox stream (site 0 on the embeddings, 1 + 2 k and 2 + 2 k in block k;
        the step counter of the device state that ``set_seed`` seeds and resets).  The two streams have the same distribution and
        DIFFERENT draws: the two modes do not train bit for bit alike at p > 0.
    forward, predict, last_hidden, calculate_loss and evaluation are the same in both modes (torch-generator dropout in training
    mode)."""

    needs_negatives = False
    needs_same_target = False
    torch_optim = True
    own_train_step = False                       # lru_step = "fused": Trainer.iteration calls train_step(input_ids, answers)
    full_logits = None                           # no dense-logits path: the rankings take last_hidden + catalogue_weight
    kernel_family = "LRU"
    model_name = "LRURec"
    layer_attr = "lru"
    step_flag = "lru_step"
    step_calls = "bsarec_lrurec"

    def __init__(self, args):
        r_min, r_max = float(getattr(args, "lru_r_min", 0.8)), float(getattr(args, "lru_r_max", 0.99))
        super().__init__(args, lambda d, std: LruLayer(d, r_min, r_max, std))

    def _param_shapes(self):
        return lrurec_param_shapes(self.LayerNorm.weight.shape[0], len(self.item_encoder.blocks))

    def _step_config(self, B: int, Lq: int):
        return L.LruRecConfig(L.LruConfig(B, Lq, self.LayerNorm.weight.shape[0]), len(self.item_encoder.blocks),
                              self.item_embeddings.num_embeddings, self.p_hidden, self.LayerNorm.eps)
