"""Mamba4Rec sibling model: an item embedding and a stack of blocks, each a selective state-space layer (an input-dependent
diagonal linear recurrence over the sequence behind a causal depthwise convolution, gated) and a position-wise feed-forward
net, trained with the full-catalogue cross-entropy of the last position.

The contract of this model is the math of its docstrings, checked against an fp64 restatement (tests/mamba_ref.py,
tests/test_mamba_cpu.py) that is itself checked against torch's autograd; it was written from the Mamba paper (Gu and Dao,
"Mamba: Linear-Time Sequence Modeling with Selective State Spaces", 2023) and the Mamba4Rec paper (Liu et al., "Mamba4Rec:
Towards Efficient Sequential Recommendation with Selective State Space Models", 2024) without their source at hand, and no
reference golden exists for it.  Where it departs from the paper's code, on purpose: the residual around the layer is kept with
one block too (the paper's code drops it at num_hidden_layers = 1), the loss is taken at the last position only (the dataset
already expands every prefix), and sequences are left-padded with the padding masked INSIDE the layer (the state is 0 until a
sequence's first item; the paper's code lets the padding's embedding run through the recurrence).  The layer runs in
libbsarec_hip.so in both directions (bsarec_mamba_fwd / bsarec_mamba_bwd, csrc/mamba.h) and the loss in the catalogue CE head
(bsarec_ce_head_fwd / _bwd); on the default path the embedding lookup, the LayerNorms, the feed-forward net and the dropout are
torch ops.  With ``mamba_step = "fused"`` the whole training step -- those parts, the item-table gradient and Adam included -- is
one C call (bsarec_mamba4rec_train_step), built by the block-model driver that LRURec's step uses too.  There is no CPU path.
The layer's and the model's plumbing, the fused mode's included, is the siblings' shared shell (_sibling.py).
"""
from __future__ import annotations

import math
from collections import OrderedDict

import torch

from . import _lib as L
from ._sibling import _BlockModel, _FlatLayer, _Holder


def default_dt_rank(width: int) -> int:
    """``--mamba_dt_rank`` when absent: 4 ceil(d / 64)."""
    return 4 * math.ceil(int(width) / 64)


def mamba_param_shapes(width: int, expand: int, d_state: int, d_conv: int, dt_rank: int) -> "OrderedDict[str, tuple]":
    """The tensors of bsarec_mamba_fwd's flat weight array, in its order (include/bsarec_hip.h)."""
    d, di, N, K, R = int(width), int(expand) * int(width), int(d_state), int(d_conv), int(dt_rank)
    return OrderedDict([("in_proj.weight", (2 * di, d)), ("conv1d.weight", (di, K)), ("conv1d.bias", (di,)),
                        ("x_proj.weight", (R + 2 * N, di)), ("dt_proj.weight", (di, R)), ("dt_proj.bias", (di,)),
                        ("A_log", (di, N)), ("D", (di,)), ("out_proj.weight", (d, di))])


def mamba4rec_param_shapes(width: int, layers: int, expand: int, d_state: int, d_conv: int,
                           dt_rank: int) -> "OrderedDict[str, tuple]":
    """The tensors of bsarec_mamba4rec_loss_grad's flat weight array under their state_dict keys, in its order
    (include/bsarec_hip.h): every parameter of Mamba4RecModel but the item table."""
    d = int(width)
    shapes = OrderedDict([("LayerNorm.weight", (d,)), ("LayerNorm.bias", (d,))])
    for k in range(int(layers)):
        blk = f"item_encoder.blocks.{k}."
        for name, shp in mamba_param_shapes(d, expand, d_state, d_conv, dt_rank).items():
            shapes[blk + "mamba." + name] = shp
        shapes[blk + "mamba.LayerNorm.weight"] = shapes[blk + "mamba.LayerNorm.bias"] = (d,)
        shapes[blk + "feed_forward.dense_1.weight"], shapes[blk + "feed_forward.dense_1.bias"] = (4 * d, d), (4 * d,)
        shapes[blk + "feed_forward.dense_2.weight"], shapes[blk + "feed_forward.dense_2.bias"] = (d, 4 * d), (d,)
        shapes[blk + "feed_forward.LayerNorm.weight"] = shapes[blk + "feed_forward.LayerNorm.bias"] = (d,)
    return shapes


class MambaLayer(_FlatLayer):
    """x [B, L, d], ids [B, L] (0 is padding; ``None``: no padding) -> out [B, L, d] on the HIP kernels, with d_inner = expand d,
    N = d_state, K = d_conv, R = dt_rank and m_t = (ids_t != 0):
      [xs_t | z_t] = in_proj(x_t);  c_t[j] = conv1d.bias[j] + sum_{k<K} conv1d.weight[j, k] (m_s xs_s[j]), s = t - K + 1 + k >= 0
      u_t = silu(c_t);  [delta_t | B_t | C_t] = x_proj(u_t);  Delta_t = softplus(dt_proj(delta_t));  A = -exp(A_log)
      m_t: h_t[j, n] = exp(Delta_t[j] A[j, n]) h_{t-1}[j, n] + Delta_t[j] B_t[n] u_t[j];  else h_t = h_{t-1};  h_{-1} = 0
      s_t[j] = sum_n C_t[n] h_t[j, n] + D[j] u_t[j];  y_t = m_t ? s_t silu(z_t) : 0;  out_t = out_proj(y_t)
    Owns ONE flat fp32 tensor in the layout of bsarec_mamba_fwd's ``weights``; ``in_proj.weight``, ``conv1d.{weight,bias}``,
    ``x_proj.weight``, ``dt_proj.{weight,bias}``, ``A_log``, ``D`` and ``out_proj.weight`` are parameters that are views of it, so
    an optimiser that updates them in place updates the array the kernels read.  ``conv1d.weight`` is [d_inner, K] (torch's
    depthwise Conv1d weight without its middle axis of 1).  The workspace carries the activations and the state checkpoints to
    the backward.

    Init: Linear weights N(0, ``std``), conv1d weight and bias U(+-K^-1/2), dt_proj.weight U(+-R^-1/2), dt_proj.bias =
    softplus^-1(dt) with dt log-uniform in [1e-3, 1e-1], A_log[j, n] = log(n + 1), D = 1."""

    _tag = "mamba"

    def __init__(self, width: int, d_state: int = 16, d_conv: int = 4, expand: int = 2, dt_rank: int | None = None,
                 std: float = 0.02):
        super().__init__()
        d = int(width)
        R = default_dt_rank(d) if dt_rank is None else int(dt_rank)
        N, K, E = int(d_state), int(d_conv), int(expand)
        if not (4 <= d <= 256 and d % 4 == 0):
            raise ValueError(f"Mamba4Rec: hidden_size {d} outside 4..256 or not a multiple of 4")
        if N not in (4, 8, 16, 32):
            raise ValueError(f"Mamba4Rec: mamba_d_state = {N}, expected 4, 8, 16 or 32")
        if not 2 <= K <= 4:
            raise ValueError(f"Mamba4Rec: mamba_d_conv = {K}, expected 2..4")
        if E not in (1, 2):
            raise ValueError(f"Mamba4Rec: mamba_expand = {E}, expected 1 or 2")
        if not (4 <= R <= 64 and R % 4 == 0):
            raise ValueError(f"Mamba4Rec: mamba_dt_rank = {R}, expected a multiple of 4 in 4..64")
        self.width, self.d_state, self.d_conv, self.expand, self.dt_rank = d, N, K, E, R
        v = self._make_flat(mamba_param_shapes(d, E, N, K, R))
        self.in_proj = _Holder(v["in_proj.weight"])
        self.conv1d = _Holder(v["conv1d.weight"], v["conv1d.bias"])
        self.x_proj = _Holder(v["x_proj.weight"])
        self.dt_proj = _Holder(v["dt_proj.weight"], v["dt_proj.bias"])
        self.register_parameter("A_log", v["A_log"])
        self.register_parameter("D", v["D"])
        self.out_proj = _Holder(v["out_proj.weight"])
        with torch.no_grad():
            for name in ("in_proj.weight", "x_proj.weight", "out_proj.weight"):
                v[name].normal_(0.0, std)
            v["conv1d.weight"].uniform_(-K ** -0.5, K ** -0.5)
            v["conv1d.bias"].uniform_(-K ** -0.5, K ** -0.5)
            v["dt_proj.weight"].uniform_(-R ** -0.5, R ** -0.5)
            dt = torch.exp(torch.rand(E * d, dtype=torch.float64) * (math.log(1e-1) - math.log(1e-3)) + math.log(1e-3))
            v["dt_proj.bias"].copy_(dt + torch.log(-torch.expm1(-dt)))
            v["A_log"].copy_(torch.log(torch.arange(1, N + 1, dtype=torch.float64)).expand(E * d, N))
            v["D"].fill_(1.0)

    def extra_repr(self):
        return (f"width={self.width}, d_state={self.d_state}, d_conv={self.d_conv}, expand={self.expand}, "
                f"dt_rank={self.dt_rank}")

    def _config(self, inputs, ids, train):
        x = self._scan_input(inputs, ids)
        cfg = L.MambaConfig(x.shape[0], x.shape[1], self.width, self.expand, self.d_state, self.d_conv, self.dt_rank)
        nbytes = L.load().bsarec_mamba_workspace_bytes(cfg, int(train))
        if nbytes < 0:
            raise ValueError(f"mamba: unsupported shape B = {x.shape[0]}, L = {x.shape[1]} (1 <= B <= 65536, 1 <= L <= 256)")
        return cfg, nbytes

    def _fwd(self, cfg, inputs, ids, train, out, ws, nbytes, stream):
        L.check(L.load().bsarec_mamba_fwd(cfg, inputs[0].data_ptr(), None if ids is None else ids.data_ptr(), self._flat.data_ptr(),
                                          train, out.data_ptr(), ws.data_ptr(), nbytes, stream), "bsarec_mamba_fwd")

    def _bwd(self, cfg, inputs, ids, flat, g, ws, nbytes, grads, dw, stream):
        L.check(L.load().bsarec_mamba_bwd(cfg, inputs[0].data_ptr(), None if ids is None else ids.data_ptr(), flat.data_ptr(),
                                          g.data_ptr(), ws.data_ptr(), nbytes, grads[0].data_ptr(), dw.data_ptr(), stream),
                "bsarec_mamba_bwd")

    def forward(self, x, ids=None):
        """Differentiable with respect to x and every parameter when autograd is recording; otherwise the train = 0 call,
        which keeps nothing."""
        return self._call((x,), None if ids is None else ids.to(torch.int64).contiguous())


class Mamba4RecModel(_BlockModel):
    """``bsarec_amd.main.MODEL_REGISTRY['mamba4rec']`` (``--model_type Mamba4Rec``).  State_dict keys: ``item_embeddings.weight``
    [V, d], ``LayerNorm.{weight,bias}``, and per block k < num_hidden_layers ``item_encoder.blocks.{k}.mamba.{in_proj.weight,
    conv1d.weight, conv1d.bias, x_proj.weight, dt_proj.weight, dt_proj.bias, A_log, D, out_proj.weight}`` (``MambaLayer``),
    ``...mamba.LayerNorm.{weight,bias}``, ``...feed_forward.{dense_1,dense_2,LayerNorm}.{weight,bias}`` (4d inner).

    forward: x = Dropout(LN(E[ids])) -- no position embedding, the recurrence carries the order; per block k:
      z = MambaLayer_k(x, ids);  a = LN(Dropout(z) + x);  x = LN(Dropout(dense_2(gelu(dense_1(a)))) + a)
    LayerNorm is TF style with eps 1e-12, gelu the erf form, every dropout ``hidden_dropout_prob`` with draws from a torch
    generator seeded by ``set_seed``.  Sequences are left-padded with id 0; padded inputs are masked inside the layer, so the
    state is 0 until a sequence's first item.
    Loss: ``cross_entropy(x[:, L - 1] @ E.T, answers)`` as one HIP node (no [B, V] logits).
    Init: Embedding and Linear weights N(0, initializer_range), Linear biases 0, LayerNorm 1 / 0, the layer's own parameters as
    ``MambaLayer`` has them with ``mamba_d_state`` (default 16), ``mamba_d_conv`` (4), ``mamba_expand`` (2) and ``mamba_dt_rank``
    (4 ceil(d / 64)).
    Departures from the paper's code: the residual around the layer is kept at num_hidden_layers = 1 too, the loss is taken at
    the last position only, and sequences are left-padded with the padding masked inside the layer.

    ``args.mamba_step`` selects how the model steps, single GPU either way:
      "torch" (the default, also when absent): calculate_loss / backward / torch.optim.Adam (``torch_optim``); the dropout masks
        are drawn from a torch generator seeded by ``set_seed``.
      "fused": ``train_step`` is ONE C call (bsarec_mamba4rec_train_step: lookup, every LayerNorm, the state-space layers, the
        feed-forward nets, the CE head, every gradient, Adam on the item table and on the flat weight array), replayed from a
        hipGraph per batch shape unless ``args.mamba_step_graph`` is False.  The model then owns ONE flat fp32 tensor in the
        layout of bsarec_mamba4rec_loss_grad's ``weights`` (``mamba4rec_param_shapes``); every parameter but the item table is a
        view of it and each ``MambaLayer._flat`` a slice of it, so state_dict keys and shapes are those of the default mode and
        checkpoints pass between the two.  The instance sets ``torch_optim = False`` and ``own_train_step = True``, which is
        what Trainer.iteration routes by.  Its dropout masks are the library's Philox stream (site 0 on the embeddings, 1 + 2 k
        and 2 + 2 k in block k; the step counter of the device state that ``set_seed`` seeds and resets).  The two streams have
        the same distribution and DIFFERENT draws: the two modes do not train bit for bit alike at p > 0.
    forward, predict, last_hidden, calculate_loss and evaluation are the same in both modes (torch-generator dropout in training
    mode)."""

    needs_negatives = False
    needs_same_target = False
    torch_optim = True
    own_train_step = False                       # mamba_step = "fused": Trainer.iteration calls train_step(input_ids, answers)
    full_logits = None                           # no dense-logits path: the rankings take last_hidden + catalogue_weight
    kernel_family = "Mamba"
    model_name = "Mamba4Rec"
    layer_attr = "mamba"
    step_flag = "mamba_step"
    step_calls = "bsarec_mamba4rec"

    def __init__(self, args):
        hyper = (int(getattr(args, "mamba_d_state", 16)), int(getattr(args, "mamba_d_conv", 4)),
                 int(getattr(args, "mamba_expand", 2)), getattr(args, "mamba_dt_rank", None))
        super().__init__(args, lambda d, std: MambaLayer(d, *hyper, std))

    def _hyper(self):
        m = self.item_encoder.blocks[0].mamba
        return m.width, m.expand, m.d_state, m.d_conv, m.dt_rank

    def _param_shapes(self):
        d, *hyper = self._hyper()
        return mamba4rec_param_shapes(d, len(self.item_encoder.blocks), *hyper)

    def _step_config(self, B: int, Lq: int):
        return L.Mamba4RecConfig(L.MambaConfig(B, Lq, *self._hyper()), len(self.item_encoder.blocks),
                                 self.item_embeddings.num_embeddings, self.p_hidden, self.LayerNorm.eps)
