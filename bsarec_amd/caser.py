"""Caser sibling model: an item embedding, a convolution block over the [L, d] embedding "image" of a sequence -- n_v vertical
filters of shape (L, 1) and, for EVERY height h = 1 .. L, n_h horizontal filters of shape (h, d) with ReLU and the maximum over
positions -- and a Linear + ReLU back to the embedding width, trained with BPR.  Item-only by default; ``args.caser_user`` adds the
user embedding of the original Caser and its second Linear + ReLU on [z1 | P[user]] (this is the one model here that reads
``user_ids``).

The contract of this model is the math of its docstrings, checked against ``torch.nn.Conv2d`` / ``F.max_pool1d`` / ``nn.Linear``
on the CPU (tests/caser_ref.py, tests/test_caser_cpu.py); no reference golden exists for it yet.  The convolution block runs in
libbsarec_hip.so in both directions (bsarec_caser_fwd / bsarec_caser_bwd, csrc/caser.h); the embedding lookup, the dropout mask,
``fc1`` and the B-row BPR head are torch ops -- unless ``args.caser_step = "fused"``, where the whole training step is one C call
(bsarec_caser_train_step, csrc/caser_step.h; with ``caser_user`` bsarec_caser_user_train_step, csrc/caser_user.h).  There is no
CPU path.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import torch
from torch import nn

from . import _fused_step as FS
from . import _lib as L
from ._sibling import _FlatLayer, _Holder, _SiblingModel, _layout, _no_cpu

CASER_NH = (4, 8, 16, 32)


def caser_param_shapes(seq_len: int, width: int, n_h: int, n_v: int) -> "OrderedDict[str, tuple]":
    """The tensors of bsarec_caser_fwd's flat weight array, in its order and with torch's Conv2d shapes (include/bsarec_hip.h)."""
    shapes = OrderedDict([("conv_v.weight", (n_v, 1, seq_len, 1)), ("conv_v.bias", (n_v,))])
    for i in range(seq_len):
        shapes[f"conv_h.{i}.weight"] = (n_h, 1, i + 1, width)
        shapes[f"conv_h.{i}.bias"] = (n_h,)
    return shapes


def caser_layout(seq_len: int, width: int, n_h: int, n_v: int):
    """({name: (offset, numel, shape)}, total floats): every tensor starts at a multiple of 4 floats (16 bytes)."""
    return _layout(caser_param_shapes(seq_len, width, n_h, n_v), 4)


class CaserConv(_FlatLayer):
    """x [B, L, d] -> z [B, n_v d + n_h L] on the HIP kernels:
      z[b, c d + j]             = sum_t conv_v.weight[c, 0, t, 0] x[b, t, j] + conv_v.bias[c]
      z[b, n_v d + i n_h + f]   = max(0, max_t (sum_{r <= i, j} conv_h.{i}.weight[f, 0, r, j] x[b, t + r, j] + conv_h.{i}.bias[f]))
    -- ``nn.Conv2d(1, n_v, (L, 1))`` and ``nn.Conv2d(1, n_h, (i + 1, d))`` -> ReLU -> max-pool over t on ``x.unsqueeze(1)``,
    concatenated.  The backward is the true derivative: a cell passes gradient only if its maximum is > 0, to the window at the
    lowest t that attains it.  Owns ONE flat fp32 tensor in the layout of bsarec_caser_fwd's ``weights`` (every tensor at a
    multiple of 4 floats); ``conv_v.weight`` / ``conv_v.bias`` / ``conv_h.{i}.weight`` / ``conv_h.{i}.bias`` are parameters that
    are views of it with torch's Conv2d shapes, so a module of ``nn.Conv2d``s under those names loads this state_dict, and the
    reverse, and an optimiser that updates them in place updates the array the kernels read.  Init is torch's Conv2d default,
    U(-1 / sqrt(fan_in), 1 / sqrt(fan_in)) for weight and bias.  The workspace carries the winning window of every cell to the
    backward."""

    _tag, _kept = "caser", "winning windows"

    def __init__(self, seq_len: int, width: int, n_h: int = 16, n_v: int = 4):
        super().__init__()
        if n_h not in CASER_NH:
            raise ValueError(f"caser_nh must be one of {CASER_NH}, got {n_h}")
        if not 1 <= n_v <= 16:
            raise ValueError(f"caser_nv must be in 1..16, got {n_v}")
        if not 1 <= seq_len <= 256:
            raise ValueError(f"Caser: max_seq_length {seq_len} outside 1..256")
        if not (4 <= width <= 256 and width % 4 == 0):
            raise ValueError(f"Caser: hidden_size {width} outside 4..256 or not a multiple of 4")
        self.seq_len, self.width, self.n_h, self.n_v = seq_len, width, n_h, n_v
        self.out_features = n_v * width + n_h * seq_len
        views = list(self._make_flat(caser_param_shapes(seq_len, width, n_h, n_v), 4).values())
        with torch.no_grad():
            for w, b in zip(views[0::2], views[1::2]):
                bound = 1.0 / math.sqrt(w[0].numel())
                w.uniform_(-bound, bound)
                b.uniform_(-bound, bound)
        self.conv_v = _Holder(views[0], views[1])
        self.conv_h = nn.ModuleList(_Holder(w, b) for w, b in zip(views[2::2], views[3::2]))

    def flat_parameters(self):
        """The parameters in the order of the flat array, as the filter banks hold them now (``load_state_dict(assign=True)``
        puts new ones there)."""
        out = [self.conv_v.weight, self.conv_v.bias]
        for c in self.conv_h:
            out += [c.weight, c.bias]
        return out

    def _config(self, inputs, extra, train):
        (x,) = inputs
        if x.dim() != 3 or x.shape[1] != self.seq_len or x.shape[2] != self.width:
            raise ValueError(f"caser: input must be [B, {self.seq_len}, {self.width}], got {tuple(x.shape)}")
        if not x.is_cuda:
            raise _no_cpu()
        self._weights_on(x)
        cfg = L.CaserConfig(x.shape[0], self.seq_len, self.width, self.n_h, self.n_v)
        nbytes = L.load().bsarec_caser_workspace_bytes(cfg, int(train))
        if nbytes < 0:
            raise ValueError(f"caser: unsupported batch B = {x.shape[0]} (1 <= B <= 65536)")
        return cfg, nbytes

    def _out_shape(self, x, extra):
        return (x.shape[0], self.out_features)

    def _fwd(self, cfg, inputs, extra, train, z, ws, nbytes, stream):
        L.check(L.load().bsarec_caser_fwd(cfg, inputs[0].data_ptr(), self._flat.data_ptr(), train, z.data_ptr(), ws.data_ptr(),
                                          nbytes, stream), "bsarec_caser_fwd")

    def _bwd(self, cfg, inputs, extra, flat, g, ws, nbytes, grads, dw, stream):
        L.check(L.load().bsarec_caser_bwd(cfg, inputs[0].data_ptr(), flat.data_ptr(), g.data_ptr(), ws.data_ptr(), nbytes,
                                          grads[0].data_ptr(), dw.data_ptr(), stream), "bsarec_caser_bwd")

    def forward(self, x):
        """[B, L, d] -> [B, n_v d + n_h L].  Differentiable with respect to x and every parameter when autograd is recording;
        otherwise the train = 0 call, which keeps nothing."""
        return self._call((x,))


class CaserModel(_SiblingModel):
    """``bsarec_amd.main.MODEL_DICT['caser']`` (``--model_type Caser``).  Parameters (the state_dict keys, in this order): ``item_embeddings.weight`` [V, d],
    ``conv.conv_v.weight`` [n_v, 1, L, 1], ``conv.conv_v.bias`` [n_v], ``conv.conv_h.{i}.weight`` [n_h, 1, i + 1, d] and
    ``conv.conv_h.{i}.bias`` [n_h] for i < L, ``fc1.weight`` [d, n_v d + n_h L], ``fc1.bias`` [d]; d = hidden_size,
    L = max_seq_length, n_h = caser_nh (default 16), n_v = caser_nv (default 4), V = item_size.

    forward: x = E[input_ids] (no position embedding, padding not masked); z = CaserConv(x); s = relu(fc1(Dropout_p(z))),
    p = hidden_dropout_prob, the mask drawn from a torch generator seeded by ``set_seed``.  ``forward`` / ``predict`` return s,
    [B, d] -- ONE state per sequence, not the [B, L, d] of the block models: Caser has no per-position output.
    Loss: BPR, mean_b -log(sigmoid(s . E[answers] - s . E[neg_answers]) + 1e-10).
    Init: Embedding and fc1 weights N(0, initializer_range), the fc1 bias 0, the filters torch's Conv2d default.
    Item-only unless ``args.caser_user`` is set (below); without it ``user_ids`` is accepted and ignored.
    The filter bank is sized by L: ``input_ids.shape[1]`` must equal ``args.max_seq_length`` (ValueError otherwise).

    ``args.caser_step`` selects how the model steps, single GPU either way:
      "torch" (the default, also when absent): calculate_loss / backward / torch.optim.Adam (``torch_optim``); the dropout mask
        is drawn from a torch generator seeded by ``set_seed``.
      "fused": ``train_step`` is ONE C call (bsarec_caser_train_step: lookup, convolution block, fc1 with its dropout, BPR head,
        every gradient, Adam on the item table, the convolution's flat array and the fc1 flat array), replayed from a hipGraph
        per batch shape unless ``args.caser_step_graph`` is False; the instance sets ``torch_optim = False`` so that
        Trainer.iteration calls it, and ``fc1.weight`` / ``fc1.bias`` are views of one flat tensor (weight, then bias).  Its
        dropout mask is the library's Philox stream (site 0, the step counter of the device state that ``set_seed`` seeds and
        resets).  The two streams have the same distribution and DIFFERENT draws: the modes do not train bit for bit alike at
        p > 0.
    calculate_loss, forward, predict and last_hidden are the same in both modes (torch-generator dropout in training mode).

    ``args.caser_user`` (default False, also when absent) is the personalised Caser, valid in both modes: two more modules, so the
    state_dict keys are ``item_embeddings.weight``, ``user_embeddings.weight`` [U, d] (U = ``args.num_users``), ``conv.*``,
    ``fc1.*``, ``fc2.weight`` [d, 2 d], ``fc2.bias`` [d] (init N(0, initializer_range) and 0).  With z1 = relu(fc1(Dropout_p(z))),
    the state is s = relu(fc2([z1 | P[user_ids]])): what forward / predict / last_hidden return and the BPR head reads.  A user id
    is the 0-based index of the user's line (what data.train_table / eval_table emit); id 0 is an ordinary row; an id outside
    [0, U) is never looked up -- its half is zero and it gets no gradient.  ``user_ids`` is then REQUIRED, [B] or [B, 1]
    (ValueError otherwise), and the instance sets ``needs_user_ids = True`` so that the Trainer passes it.  In fused mode the
    step is bsarec_caser_user_train_step, ``fc2.weight`` / ``fc2.bias`` are views of one flat tensor like fc1's, and Adam runs on
    five arrays.  Without the flag the model is what it was: same parameters, same bits, same state_dict."""

    needs_negatives = True
    needs_same_target = False
    needs_user_ids = False                       # True on an instance with caser_user: Trainer passes user_ids
    torch_optim = True
    kernel_family = "Caser"                      # Trainer's messages
    model_name = "Caser"

    def __init__(self, args):
        super().__init__(args)
        mode = getattr(args, "caser_step", "torch")
        if mode not in ("torch", "fused"):
            raise ValueError(f"caser_step must be 'torch' or 'fused', got {mode!r}")
        self.caser_step = mode
        if mode == "fused":
            self.torch_optim = False                      # Trainer.iteration: the pairwise branch, model.train_step
        self._fc_flat = None                              # fused: fc1.weight [d, F] then fc1.bias [d]
        self._fc2_flat = None                             # fused with caser_user: fc2.weight [d, 2 d] then fc2.bias [d]
        self.caser_user = bool(getattr(args, "caser_user", False))
        d, Lq = int(args.hidden_size), int(args.max_seq_length)
        self.item_embeddings = nn.Embedding(int(args.item_size), d)
        if self.caser_user:
            U = getattr(args, "num_users", None)
            if U is None or int(U) < 1:
                raise ValueError(f"Caser: caser_user needs args.num_users >= 1, got {U!r}")
            self.needs_user_ids = True
            self.user_embeddings = nn.Embedding(int(U), d)
        self.conv = CaserConv(Lq, d, int(getattr(args, "caser_nh", 16)), int(getattr(args, "caser_nv", 4)))
        self.fc1 = nn.Linear(self.conv.out_features, d)
        if self.caser_user:
            self.fc2 = nn.Linear(2 * d, d)
        self.p_drop = float(args.hidden_dropout_prob)
        if not 0.0 <= self.p_drop < 1.0:
            raise ValueError(f"hidden_dropout_prob must be in [0, 1), got {self.p_drop}")
        std = float(args.initializer_range)
        with torch.no_grad():
            self.item_embeddings.weight.normal_(0.0, std)
            self.fc1.weight.normal_(0.0, std)
            self.fc1.bias.zero_()
            if self.caser_user:
                self.user_embeddings.weight.normal_(0.0, std)
                self.fc2.weight.normal_(0.0, std)
                self.fc2.bias.zero_()
        self.reflatten()

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        self.reflatten()
        return out

    def reflatten(self):
        """Makes the convolution's parameters views of its flat tensor again and, with ``caser_step = "fused"``, ``fc1.weight``
        and ``fc1.bias`` views of one flat tensor, weight then bias (after ``.to()`` / ``.cuda()`` / ``load_state_dict(assign=True)``
        gave each its own storage).  The fused step's buffers go with a storage that changed."""
        self.conv.reflatten()
        if self.caser_step != "fused":
            return
        self._fc_flat = self._flat_linear(self.fc1, self._fc_flat)
        if self.caser_user:                               # fc2 alike: weight [d, 2 d], then bias [d]
            self._fc2_flat = self._flat_linear(self.fc2, self._fc2_flat)

    def _flat_linear(self, lin, flat):
        """``lin.weight`` / ``lin.bias`` as views of one flat tensor, weight then bias: ``flat`` if they still are, else a new one
        with their values (and the fused step's buffers go)."""
        w, b = lin.weight, lin.bias
        nw = w.numel()
        if (flat is not None and flat.device == w.device == b.device and w.data_ptr() == flat.data_ptr()
                and b.data_ptr() == flat.data_ptr() + 4 * nw and w.is_contiguous()):
            return flat
        with torch.no_grad():
            flat = torch.empty(nw + b.numel(), dtype=torch.float32, device=w.device)
            flat[:nw] = w.detach().reshape(-1).to(torch.float32)
            flat[nw:] = b.detach().reshape(-1).to(torch.float32)
            w.data = flat[:nw].view(w.shape)
            b.data = flat[nw:].view(b.shape)
            w.grad = b.grad = None
        self._fused = None
        return flat

    def _check_ids(self, input_ids):
        if input_ids.dim() != 2 or input_ids.shape[1] != self.conv.seq_len:
            raise ValueError(f"Caser: input_ids must be [B, max_seq_length = {self.conv.seq_len}] (the filter bank is sized by it), "
                             f"got {tuple(input_ids.shape)}")

    def _users(self, user_ids, input_ids):
        """caser_user: ``user_ids`` as int64 [B] on the device of ``input_ids`` [B, L]; [B] or [B, 1] only (ValueError: missing,
        another shape).  None without the flag: the ids are ignored.  Stands before the device check of every public call."""
        if not self.caser_user:
            return None
        if user_ids is None:
            raise ValueError("Caser: caser_user needs user_ids")
        B = input_ids.shape[0] if input_ids.dim() else -1
        if tuple(user_ids.shape) not in ((B,), (B, 1)):
            raise ValueError(f"Caser: user_ids must be [B] or [B, 1] with B = {B}, got {tuple(user_ids.shape)}")
        return user_ids.to(device=input_ids.device, dtype=torch.int64).reshape(-1)

    def _state(self, input_ids, train: bool, users=None):
        z1 = torch.relu(self.fc1(self._drop(self.conv(self.item_embeddings(input_ids)), self.p_drop, train)))
        if not self.caser_user:
            return z1
        U = self.user_embeddings.num_embeddings
        inside = (users >= 0) & (users < U)               # an id outside [0, U): never looked up, a zero half, no gradient
        pu = self.user_embeddings(users.clamp(0, U - 1)) * inside.unsqueeze(-1).to(z1.dtype)
        return torch.relu(self.fc2(torch.cat([z1, pu], dim=-1)))

    def forward(self, input_ids, user_ids=None, all_sequence_output=False):
        """[B, L] ids -> s [B, d].  ``all_sequence_output`` is accepted and ignored, and so is ``user_ids`` unless
        ``caser_user`` is set."""
        users = self._users(user_ids, input_ids)
        self._require_gpu(input_ids)
        return self._state(input_ids, self.training, users)

    def last_hidden(self, input_ids, user_ids=None) -> torch.Tensor:
        """[B, d]: the eval-mode s (the bits of ``forward`` in eval mode), no gradient."""
        users = self._users(user_ids, input_ids)
        self._require_gpu(input_ids)
        with torch.no_grad():
            return self._state(input_ids, False, users)

    def calculate_loss(self, input_ids, answers, neg_answers=None, same_target=None, user_ids=None):
        """BPR on s: a 0-d tensor; ``.backward()`` fills every parameter's grad."""
        if neg_answers is None:
            raise ValueError("Caser's loss needs neg_answers")
        users = self._users(user_ids, input_ids)
        self._require_gpu(input_ids)
        s = self._state(input_ids, self.training, users)
        pos = self.item_embeddings(answers.to(s.device).reshape(-1))
        neg = self.item_embeddings(neg_answers.to(s.device).reshape(-1))
        diff = (s * pos).sum(-1) - (s * neg).sum(-1)
        return -torch.log(torch.sigmoid(diff) + 1e-10).mean()

    # ---- the fused step (caser_step = "fused"; bsarec_caser_loss_grad / bsarec_caser_train_step; host side: _fused_step.py) ----
    def _step_buffers(self):
        """What the fused step owns beside the parameters: the device step state (seed, step counter, Adam t), the three gradient
        arrays, the Adam moments of the item table ("E"), of the convolution's flat array ("W") and of the fc1 flat array ("F"),
        and per batch shape a workspace, static id buffers and a captured graph.  Built on first use; dropped by ``.to()`` /
        ``reflatten()`` (a new parameter storage).  With ``caser_user`` two more arrays, the user table ("P") and the fc2 flat
        array ("G"), each with its gradient and moments (dP / mP / vP, dG / mG / vG), and a static ``users`` buffer per batch
        shape."""
        if self.caser_step != "fused":
            raise RuntimeError("Caser: the fused step's buffers exist only with caser_step = 'fused'")
        self._require_gpu()
        self.reflatten()
        E, flat, fc = self.item_embeddings.weight.data, self.conv._flat, self._fc_flat
        if flat.device != E.device or fc.device != E.device or not E.is_contiguous() or E.dtype != torch.float32:
            raise RuntimeError("caser: the item table, the filters and fc1 must be contiguous fp32 on one device")
        arrays = [("E", E), ("W", flat), ("F", fc)]
        if self.caser_user:
            P, fc2 = self.user_embeddings.weight.data, self._fc2_flat
            if P.device != E.device or fc2.device != E.device or not P.is_contiguous() or P.dtype != torch.float32:
                raise RuntimeError("caser: the user table and fc2 must be contiguous fp32 on the item table's device")
            arrays += [("P", P), ("G", fc2)]
        self._fused = FS.buffers(self._fused, arrays, self._stream_seed())
        return self._fused

    def _slot(self, f, B: int):
        s = f["slots"].get(B)
        if s is None:
            c = self.conv
            cfg = L.CaserStepConfig(L.CaserConfig(B, c.seq_len, c.width, c.n_h, c.n_v), self.item_embeddings.num_embeddings,
                                    self.p_drop)
            if self.caser_user:
                cfg = L.CaserUserStepConfig(cfg, self.user_embeddings.num_embeddings)
                nbytes = L.load().bsarec_caser_user_step_workspace_bytes(cfg)
            else:
                nbytes = L.load().bsarec_caser_step_workspace_bytes(cfg)
            if nbytes < 0:
                raise ValueError(f"caser: unsupported step shape B = {B}, dropout = {self.p_drop} (1 <= B <= 65536, 0 <= p < 1)")
            s = FS.slot(f, B, cfg, nbytes, (B, c.seq_len), ("users",) if self.caser_user else ())
        return s

    def _fill(self, s, input_ids, answers, neg_answers, users=None):
        if neg_answers is None:
            raise ValueError("Caser's loss needs neg_answers")
        s["ids"].copy_(input_ids)
        s["ans"].copy_(answers.reshape(-1))
        s["neg"].copy_(neg_answers.reshape(-1))
        if users is not None:
            s["users"].copy_(users)
        return s

    def _loss_grad(self, f, s, train: bool):
        ptr = lambda t: t.data_ptr()
        tail = (ptr(f["state"]), int(train), ptr(s["loss"]))
        if self.caser_user:
            L.check(L.load().bsarec_caser_user_loss_grad(
                s["cfg"], ptr(f["E"]), ptr(f["P"]), ptr(f["W"]), ptr(f["F"]), ptr(f["G"]), ptr(s["ids"]), ptr(s["users"]),
                ptr(s["ans"]), ptr(s["neg"]), *tail, ptr(f["dE"]), ptr(f["dP"]), ptr(f["dW"]), ptr(f["dF"]), ptr(f["dG"]),
                ptr(s["ws"]), s["nbytes"], FS.stream(f)), "bsarec_caser_user_loss_grad")
            return
        L.check(L.load().bsarec_caser_loss_grad(
            s["cfg"], ptr(f["E"]), ptr(f["W"]), ptr(f["F"]), ptr(s["ids"]), ptr(s["ans"]), ptr(s["neg"]), *tail, ptr(f["dE"]),
            ptr(f["dW"]), ptr(f["dF"]), ptr(s["ws"]), s["nbytes"], FS.stream(f)), "bsarec_caser_loss_grad")

    def loss_and_grads(self, input_ids, answers, neg_answers, train: bool = True, user_ids=None):
        """The BPR loss (0-d tensor) and {state_dict key: gradient} of one batch through bsarec_caser_loss_grad
        (bsarec_caser_user_loss_grad with ``caser_user``, which needs ``user_ids``), no update.
        ``train``: draw the next dropout mask of the device stream (the step counter advances); else no dropout."""
        if self.caser_step != "fused":
            raise RuntimeError("Caser: loss_and_grads is the fused step's (caser_step = 'fused')")
        users = self._users(user_ids, input_ids)
        self._require_gpu(input_ids)
        f = self._step_buffers()
        s = self._fill(self._slot(f, int(input_ids.shape[0])), input_ids, answers, neg_answers, users)
        self._loss_grad(f, s, train)
        grads = OrderedDict([("item_embeddings.weight", f["dE"].clone())])
        if self.caser_user:
            grads["user_embeddings.weight"] = f["dP"].clone()
        for name, (o, n, shp) in self.conv._slices.items():
            grads["conv." + name] = f["dW"][o:o + n].view(shp).clone()
        for name, lin, g in (("fc1", self.fc1, "dF"),) + ((("fc2", self.fc2, "dG"),) if self.caser_user else ()):
            nw = lin.weight.numel()
            grads[name + ".weight"] = f[g][:nw].view(lin.weight.shape).clone()
            grads[name + ".bias"] = f[g][nw:].clone()
        return s["loss"].clone(), grads

    def _train_step(self, f, s):
        ptr = lambda t: t.data_ptr()
        adams = FS.adam_structs(f, self.args)             # in the arrays' order: items, weights, fc (, users, fc2)
        tail = (ptr(f["state"]), ptr(s["loss"]), ptr(s["ws"]), s["nbytes"], FS.stream(f))
        if self.caser_user:
            items, weights, fc, users, fc2 = adams
            L.check(L.load().bsarec_caser_user_train_step(
                s["cfg"], ptr(s["ids"]), ptr(s["users"]), ptr(s["ans"]), ptr(s["neg"]), items, users, weights, fc, fc2, *tail),
                "bsarec_caser_user_train_step")
            return
        L.check(L.load().bsarec_caser_train_step(s["cfg"], ptr(s["ids"]), ptr(s["ans"]), ptr(s["neg"]), *adams, *tail),
                "bsarec_caser_train_step")

    def train_step(self, input_ids, answers, neg_answers=None, same_target=None, user_ids=None):
        """caser_step = "fused": one optimisation step in one C call -- the step counter, the lookup, the convolution block, fc1
        with its Philox dropout, the BPR head, every gradient, Adam (``args.lr``, ``adam_beta1``, ``adam_beta2``,
        ``weight_decay``) on the three arrays, in place.  Returns the mean loss as a 0-d device tensor (no host sync; the next
        step overwrites it).  The call is captured once per batch shape over static id buffers and replayed -- the mask and
        Adam's t advance on the device, and the capture is one linear chain on one stream, so it has no parallel branches to
        replay; ``args.caser_step_graph = False`` calls eagerly instead.  With ``caser_user`` the call is
        bsarec_caser_user_train_step (five arrays) and ``user_ids`` goes into a static buffer beside the ids."""
        if self.caser_step != "fused":
            raise self._torch_steps(" unless caser_step = 'fused'")
        users = self._users(user_ids, input_ids)
        self._require_gpu(input_ids)
        f = self._step_buffers()
        s = self._fill(self._slot(f, int(input_ids.shape[0])), input_ids, answers, neg_answers, users)
        return FS.train_step(f, s, self.args, getattr(self.args, "caser_step_graph", True), self._loss_grad, self._train_step)
