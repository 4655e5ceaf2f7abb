"""GRU4Rec sibling model: an item embedding, a stack of bias-free GRU layers and a Linear back to the embedding width, trained
with BPR at the last position.

The contract of this model is the math of its docstrings, checked against ``torch.nn.Embedding`` / ``nn.GRU(bias=False)`` /
``nn.Linear`` on the CPU (tests/gru_ref.py, tests/test_gru_cpu.py); no reference golden exists for it yet.  Everything between
the dropped-out embeddings and the output runs in libbsarec_hip.so in both directions (bsarec_gru_fwd / bsarec_gru_bwd,
csrc/gru.h); on the default path the embedding lookup, the dropout mask and the B-row BPR head are torch ops.  With
``gru_step = "fused"`` the whole training step -- those parts, the item-table gradient and Adam included -- is one C call
(bsarec_gru4rec_train_step, csrc/pair_step.h).  ``gru_loss`` / ``gru_negatives`` replace the pairwise BPR loss by
cross-entropy, TOP1 or BPR-max over mini-batch negatives (csrc/gru4rec_cand.h inside the fused step, ``cand_head_loss`` in torch
ops on the default path).  There is no CPU path.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import torch
from torch import nn

from . import _fused_step as FS
from . import _lib as L
from ._sibling import _FlatLayer, _Holder, _SiblingModel, _no_cpu

GRU_HIDDEN = (32, 64, 96, 128)


def gru_param_shapes(input_size: int, hidden_size: int, num_layers: int, out_size: int) -> "OrderedDict[str, tuple]":
    """The tensors of bsarec_gru_fwd's flat weight array, in its order (include/bsarec_hip.h)."""
    shapes = OrderedDict()
    for k in range(num_layers):
        shapes[f"weight_ih_l{k}"] = (3 * hidden_size, input_size if k == 0 else hidden_size)
        shapes[f"weight_hh_l{k}"] = (3 * hidden_size, hidden_size)
    if out_size:
        shapes["out_weight"] = (out_size, hidden_size)
        shapes["out_bias"] = (out_size,)
    return shapes


class GruStack(_FlatLayer):
    """``nn.GRU(input_size, hidden_size, num_layers, bias=False, batch_first=True)`` with h_0 = 0 and, when ``out_size`` is
    not 0, ``nn.Linear(hidden_size, out_size)`` on top, on the HIP kernels.  Owns ONE flat fp32 tensor in the layout of
    bsarec_gru_fwd's ``weights``; ``weight_ih_l{k}`` / ``weight_hh_l{k}`` are parameters that are views of it, so an optimiser
    that updates them in place updates the array the kernels read.  ``out_weight`` / ``out_bias`` are views of its tail: plain
    attributes here, for the owner to register under its own names (GRU4RecModel: ``dense.weight`` / ``dense.bias``).  The
    workspace carries the forward's activations to the backward."""

    _tag = "gru"

    def __init__(self, input_size: int, hidden_size: int, num_layers: int, out_size: int = 0):
        super().__init__()
        if hidden_size not in GRU_HIDDEN:
            raise ValueError(f"gru_hidden_size must be one of {GRU_HIDDEN}, got {hidden_size}")
        if not 1 <= num_layers <= 4:
            raise ValueError(f"GRU stack: 1..4 layers, got {num_layers}")
        for name, v in (("input", input_size), ("output", out_size)):
            if not (v == 0 and name == "output") and not (4 <= v <= 256 and v % 4 == 0):
                raise ValueError(f"GRU stack: {name} size {v} outside 4..256 or not a multiple of 4")
        self.input_size, self.hidden_size, self.num_layers, self.out_size = input_size, hidden_size, num_layers, out_size
        bound = 1.0 / math.sqrt(hidden_size)
        for name, p in self._make_flat(gru_param_shapes(input_size, hidden_size, num_layers, out_size)).items():
            if name.startswith("weight_"):
                self.register_parameter(name, p)
                with torch.no_grad():
                    p.uniform_(-bound, bound)                 # torch's default for nn.GRU

    @property
    def out_weight(self):
        return self._views.get("out_weight")

    @property
    def out_bias(self):
        return self._views.get("out_bias")

    def _apply(self, fn, recurse=True):
        with torch.no_grad():
            for name, p in self._views.items():
                if not name.startswith("weight_"):           # registered by the owner: moved here too, so the views stay together
                    p.data = fn(p.data)
        return super()._apply(fn, recurse)

    def _config(self, inputs, last_only, train):
        (x,) = inputs
        if x.dim() != 3 or x.shape[2] != self.input_size:
            raise ValueError(f"gru: input must be [B, L, {self.input_size}], got {tuple(x.shape)}")
        if not x.is_cuda:
            raise _no_cpu()
        self._weights_on(x)
        cfg = L.GruConfig(x.shape[0], x.shape[1], self.input_size, self.hidden_size, self.num_layers, self.out_size)
        nbytes = L.load().bsarec_gru_workspace_bytes(cfg, int(train))
        if nbytes < 0:
            raise ValueError(f"gru: unsupported shape B = {x.shape[0]}, L = {x.shape[1]} (1 <= B <= 65536, 1 <= L <= 256)")
        return cfg, nbytes

    def _out_shape(self, x, last_only):
        w = self.out_size or self.hidden_size
        return (x.shape[0], w) if last_only else (x.shape[0], x.shape[1], w)

    def _fwd(self, cfg, inputs, last_only, train, out, ws, nbytes, stream):
        L.check(L.load().bsarec_gru_fwd(cfg, inputs[0].data_ptr(), self._flat.data_ptr(), train, int(last_only), out.data_ptr(),
                                        ws.data_ptr(), nbytes, stream), "bsarec_gru_fwd")

    def _bwd(self, cfg, inputs, last_only, flat, g, ws, nbytes, grads, dw, stream):
        L.check(L.load().bsarec_gru_bwd(cfg, inputs[0].data_ptr(), flat.data_ptr(), int(last_only), g.data_ptr(), ws.data_ptr(),
                                        nbytes, grads[0].data_ptr(), dw.data_ptr(), stream), "bsarec_gru_bwd")

    def forward(self, x, last_only: bool = False):
        """[B, L, input] -> [B, L, out] (``last_only``: [B, out], position L - 1).  Differentiable with respect to x and every
        parameter when autograd is recording; otherwise the train = 0 call, which keeps nothing."""
        return self._call((x,), bool(last_only))


GRU_LOSSES = ("bpr",) + tuple(L.GRU4REC_LOSSES)
GRU_NEGATIVES = ("pair",) + tuple(L.GRU4REC_CANDIDATES)


def cand_head_loss(s, E, answers, neg_answers, loss: str, negatives: str, bpreg: float = 1.0):
    """The heads over candidates shared by the batch (bsarec_gru4rec_cand_head, include/bsarec_hip.h) in torch ops, differentiable
    in ``s`` [B, d] and ``E`` [V, d]: the loss of ``gru_step = "torch"`` and the cross-check of the HIP head.  The candidates are
    the batch's answers ("in_batch") and behind them the negatives ("in_batch+sampled"); row b's positive is column b, its
    negatives are the columns whose item is not answers[b]; a row without negatives has loss 0."""
    cand = answers if negatives == "in_batch" else torch.cat([answers, neg_answers])
    return cand_scores_loss(s @ E[cand].T, cand, answers, loss, bpreg)


def cand_scores_loss(r, cand, answers, loss: str, bpreg: float = 1.0):
    """``cand_head_loss`` from the scores r [B, C] of the candidates ``cand`` [C] (the first B are ``answers``)."""
    B = r.shape[0]
    pos = r[:, :B].diagonal().unsqueeze(1)
    neg = cand.unsqueeze(0) != answers.unsqueeze(1)            # M_b
    m = neg.sum(1)
    some = m > 0
    if loss == "ce":
        keep = neg | torch.eye(B, r.shape[1], dtype=torch.bool, device=r.device)
        rows = torch.logsumexp(r.masked_fill(~keep, -math.inf), 1) - pos.squeeze(1)
    elif loss == "top1":
        rows = ((torch.sigmoid(r - pos) + torch.sigmoid(r * r)) * neg).sum(1) / m.clamp(min=1)
    else:
        x = torch.where(some.unsqueeze(1), r.masked_fill(~neg, -math.inf), torch.zeros_like(r))
        p = torch.softmax(x, 1)
        rows = -torch.log((p * torch.sigmoid(pos - r)).sum(1) + 1e-10) + bpreg * (p * r * r).sum(1)
    return torch.where(some, rows, torch.zeros_like(rows)).mean()


class GRU4RecModel(_SiblingModel):
    """``MODEL_DICT['gru4rec']``.  Parameters (the state_dict keys, in this order): ``item_embeddings.weight`` [V, d],
    ``gru_layers.weight_ih_l{k}`` [3H, d or H] and ``gru_layers.weight_hh_l{k}`` [3H, H] for k < N, ``dense.weight`` [d, H],
    ``dense.bias`` [d]; d = hidden_size, H = gru_hidden_size (default 64), N = num_hidden_layers, V = item_size.  A model of
    ``nn.Embedding(V, d)``, ``nn.GRU(d, H, N, bias=False, batch_first=True)`` and ``nn.Linear(H, d)`` under those attribute
    names loads this state_dict, and the reverse.

    forward: x = Dropout_p(E[input_ids]), p = hidden_dropout_prob; y = GRU(x) with h_0 = 0 over all L positions (padding is not
    masked), no dropout between layers; out = y . dense.weight^T + dense.bias, [B, L, d].
    Loss: BPR at the last position, mean_b -log(sigmoid(s . E[answers] - s . E[neg_answers]) + 1e-10) with s = out[:, L - 1].
    Init: Embedding and Linear weights N(0, initializer_range), the Linear bias 0, GRU weights U(-1 / sqrt(H), 1 / sqrt(H)).

    ``args.gru_step`` selects how the model steps, single GPU either way:
      "torch" (the default, also when absent): calculate_loss / backward / torch.optim.Adam (``torch_optim``); the dropout mask
        is drawn from a torch generator seeded by ``set_seed``.
      "fused": ``train_step`` is ONE C call (bsarec_gru4rec_train_step: lookup, dropout, GRU, BPR head, every gradient, Adam on
        the item table and on the GRU flat array), replayed from a hipGraph per batch shape unless ``args.gru_step_graph`` is
        False; the instance sets ``torch_optim = False`` so that Trainer.iteration calls it.  Its dropout mask is the library's
        Philox stream (site 0, the step counter of the device state that ``set_seed`` seeds and resets).  The two streams have
        the same distribution and DIFFERENT draws: the two modes do not train bit for bit alike at p > 0.
    calculate_loss, forward, predict and last_hidden are the same in both modes (torch-generator dropout in training mode).

    ``args.gru_loss`` / ``args.gru_negatives`` / ``args.gru_bpreg`` select the loss at the last position.  "bpr" with "pair" (the
    defaults, also when absent) is the pairwise loss above.  "ce", "top1" and "bpr_max" go with "in_batch" (the other rows'
    answers are a row's negatives) or "in_batch+sampled" (those and every row's neg_answers): the heads of
    bsarec_gru4rec_cand_head (include/bsarec_hip.h; ``cand_head_loss`` is their math in torch ops), ``gru_bpreg`` (default 1.0)
    the weight of BPR-max's score regulariser.  With ``gru_step = "fused"`` the step calls bsarec_gru4rec_cand_train_step (the
    head as HIP kernels inside the one C call), with "torch" calculate_loss forms the loss with torch ops.  Any other pair of
    loss and negatives raises ValueError."""

    needs_negatives = True
    needs_same_target = False
    torch_optim = True
    model_name = "GRU4Rec"

    def __init__(self, args):
        super().__init__(args)
        mode = getattr(args, "gru_step", "torch")
        if mode not in ("torch", "fused"):
            raise ValueError(f"gru_step must be 'torch' or 'fused', got {mode!r}")
        self.gru_step = mode
        loss, negatives = getattr(args, "gru_loss", "bpr"), getattr(args, "gru_negatives", "pair")
        if loss not in GRU_LOSSES:
            raise ValueError(f"gru_loss must be one of {GRU_LOSSES}, got {loss!r}")
        if negatives not in GRU_NEGATIVES:
            raise ValueError(f"gru_negatives must be one of {GRU_NEGATIVES}, got {negatives!r}")
        if (loss == "bpr") != (negatives == "pair"):
            raise ValueError(f"gru_loss = {loss!r} does not go with gru_negatives = {negatives!r}: 'bpr' takes 'pair', and "
                             f"{GRU_LOSSES[1:]} take {GRU_NEGATIVES[1:]}")
        bpreg = float(getattr(args, "gru_bpreg", 1.0))
        if not bpreg >= 0.0:
            raise ValueError(f"gru_bpreg must be >= 0, got {bpreg}")
        self.gru_loss, self.gru_negatives, self.gru_bpreg = loss, negatives, bpreg
        # the head over shared candidates (bsarec_gru4rec_head_t), or None: the pairwise BPR head
        self._head = None if loss == "bpr" else L.Gru4RecHead(L.GRU4REC_LOSSES[loss], L.GRU4REC_CANDIDATES[negatives], bpreg)
        if mode == "fused":
            self.torch_optim = False                      # Trainer.iteration: the pairwise branch, model.train_step
        d, H = int(args.hidden_size), int(getattr(args, "gru_hidden_size", 64))
        self.item_embeddings = nn.Embedding(int(args.item_size), d)
        self.gru_layers = GruStack(d, H, int(args.num_hidden_layers), d)
        self.dense = _Holder(self.gru_layers.out_weight, self.gru_layers.out_bias)     # the projection runs in bsarec_gru_fwd
        self.p_drop = float(args.hidden_dropout_prob)
        std = float(args.initializer_range)
        with torch.no_grad():
            self.item_embeddings.weight.normal_(0.0, std)
            self.dense.weight.normal_(0.0, std)
            self.dense.bias.zero_()

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        self.gru_layers.reflatten()                       # ``dense`` moved its two views after the stack had flattened itself
        return out

    def _check_ids(self, input_ids):
        pass                                              # the stack checks its [B, L, d] input, the fused step its ids (_fill)

    def _embed(self, input_ids, train: bool):
        return self._drop(self.item_embeddings(input_ids), self.p_drop, train)

    def forward(self, input_ids, user_ids=None, all_sequence_output=False):
        """[B, L] ids -> [B, L, d].  ``all_sequence_output`` is accepted and ignored."""
        self._require_gpu(input_ids)
        return self.gru_layers(self._embed(input_ids, self.training))

    def last_hidden(self, input_ids) -> torch.Tensor:
        """[B, d]: the eval-mode output at position L - 1 (the bits of ``forward`` in eval mode at that row), no gradient."""
        self._require_gpu(input_ids)
        with torch.no_grad():
            return self.gru_layers(self._embed(input_ids, False), last_only=True)

    def calculate_loss(self, input_ids, answers, neg_answers=None, same_target=None, user_ids=None):
        """BPR at the last position: a 0-d tensor; ``.backward()`` fills every parameter's grad."""
        if neg_answers is None:
            raise ValueError("GRU4Rec's loss needs neg_answers")
        self._require_gpu(input_ids)
        s = self.gru_layers(self._embed(input_ids, self.training), last_only=True)
        dev = s.device
        if self._head is not None:
            return cand_head_loss(s, self.item_embeddings.weight, answers.to(dev).reshape(-1), neg_answers.to(dev).reshape(-1),
                                  self.gru_loss, self.gru_negatives, self.gru_bpreg)
        pos = self.item_embeddings(answers.to(dev))
        neg = self.item_embeddings(neg_answers.to(dev))
        diff = (s * pos).sum(-1) - (s * neg).sum(-1)
        return -torch.log(torch.sigmoid(diff) + 1e-10).mean()

    # ---- the fused step (gru_step = "fused"; bsarec_gru4rec_loss_grad / bsarec_gru4rec_train_step; host side: _fused_step.py) ----
    def _step_buffers(self):
        """What the fused step owns beside the parameters: the device step state (seed, step counter, Adam t), both gradient
        arrays, the Adam moments of the item table ("E") and of the GRU flat array ("W"), and per batch shape a workspace, static
        id buffers and a captured graph.  Built on first use; dropped by ``.to()`` / ``reflatten()`` (a new parameter storage)."""
        self._require_gpu()
        self.gru_layers.reflatten()
        E, flat = self.item_embeddings.weight.data, self.gru_layers._flat
        if flat.device != E.device or not E.is_contiguous() or E.dtype != torch.float32:
            raise RuntimeError("gru4rec: the item table and the GRU weights must be contiguous fp32 on one device")
        self._fused = FS.buffers(self._fused, [("E", E), ("W", flat)], self._stream_seed())
        return self._fused

    def _slot(self, f, B: int, Lq: int):
        s = f["slots"].get((B, Lq))
        if s is None:
            g = self.gru_layers
            cfg = L.Gru4RecConfig(L.GruConfig(B, Lq, g.input_size, g.hidden_size, g.num_layers, g.out_size),
                                  self.item_embeddings.num_embeddings, self.p_drop)
            if self._head is None:
                nbytes = L.load().bsarec_gru4rec_workspace_bytes(cfg)
            else:
                nbytes = L.load().bsarec_gru4rec_cand_workspace_bytes(cfg, self._head)
            if nbytes < 0:
                raise ValueError(f"gru4rec: unsupported step shape B = {B}, L = {Lq}, dropout = {self.p_drop} "
                                 "(1 <= B <= 65536, 1 <= L <= 256, 0 <= p < 1" +
                                 ("" if self._head is None else
                                  f", at most {L.GRU4REC_CAND_MAX} candidates: {self._head.candidates} B") + ")")
            s = FS.slot(f, (B, Lq), cfg, nbytes, (B, Lq))
        return s

    def _fill(self, s, input_ids, answers, neg_answers):
        if neg_answers is None:
            raise ValueError("GRU4Rec's loss needs neg_answers")
        if input_ids.dim() != 2:
            raise ValueError(f"gru4rec: input_ids must be [B, L], got {tuple(input_ids.shape)}")
        s["ids"].copy_(input_ids)
        s["ans"].copy_(answers.reshape(-1))
        s["neg"].copy_(neg_answers.reshape(-1))
        return s

    def _loss_grad(self, f, s, train: bool):
        call = (s["cfg"], f["E"].data_ptr(), f["W"].data_ptr(), s["ids"].data_ptr(), s["ans"].data_ptr(), s["neg"].data_ptr(),
                f["state"].data_ptr(), int(train), s["loss"].data_ptr(), f["dE"].data_ptr(), f["dW"].data_ptr(), s["ws"].data_ptr(),
                s["nbytes"], FS.stream(f))
        if self._head is None:
            L.check(L.load().bsarec_gru4rec_loss_grad(*call), "bsarec_gru4rec_loss_grad")
        else:
            L.check(L.load().bsarec_gru4rec_cand_loss_grad(*call, self._head), "bsarec_gru4rec_cand_loss_grad")

    def loss_and_grads(self, input_ids, answers, neg_answers, train: bool = True):
        """The BPR loss (0-d tensor) and {state_dict key: gradient} of one batch through bsarec_gru4rec_loss_grad, no update.
        ``train``: draw the next dropout mask of the device stream (the step counter advances); else no dropout."""
        self._require_gpu(input_ids)
        f = self._step_buffers()
        s = self._fill(self._slot(f, int(input_ids.shape[0]), int(input_ids.shape[1])), input_ids, answers, neg_answers)
        self._loss_grad(f, s, train)
        grads = OrderedDict([("item_embeddings.weight", f["dE"].clone())])
        names = {"out_weight": "dense.weight", "out_bias": "dense.bias"}
        for name, (o, n, shp) in self.gru_layers._slices.items():
            grads[names.get(name, "gru_layers." + name)] = f["dW"][o:o + n].view(shp).clone()
        return s["loss"].clone(), grads

    def _train_step(self, f, s):
        items, weights = FS.adam_structs(f, self.args)
        call = (s["cfg"], s["ids"].data_ptr(), s["ans"].data_ptr(), s["neg"].data_ptr(), items, weights, f["state"].data_ptr(),
                s["loss"].data_ptr(), s["ws"].data_ptr(), s["nbytes"], FS.stream(f))
        if self._head is None:
            L.check(L.load().bsarec_gru4rec_train_step(*call), "bsarec_gru4rec_train_step")
        else:
            L.check(L.load().bsarec_gru4rec_cand_train_step(*call, self._head), "bsarec_gru4rec_cand_train_step")

    def train_step(self, input_ids, answers, neg_answers=None, same_target=None):
        """gru_step = "fused": one optimisation step in one C call -- the step counter, lookup + Philox dropout, the GRU stack,
        the BPR head, every gradient, Adam (``args.lr``, ``adam_beta1``, ``adam_beta2``, ``weight_decay``) on the item table and
        on the GRU flat array, in place.  Returns the mean loss as a 0-d device tensor (no host sync; the next step overwrites
        it).  The call is captured once per batch shape over static id buffers and replayed -- the mask and Adam's t advance on
        the device, and the capture is one linear chain on one stream, so it has no parallel branches to replay;
        ``args.gru_step_graph = False`` calls eagerly instead."""
        if self.gru_step != "fused":
            raise self._torch_steps()
        self._require_gpu(input_ids)
        f = self._step_buffers()
        s = self._fill(self._slot(f, int(input_ids.shape[0]), int(input_ids.shape[1])), input_ids, answers, neg_answers)
        return FS.train_step(f, s, self.args, getattr(self.args, "gru_step_graph", True), self._loss_grad, self._train_step)
