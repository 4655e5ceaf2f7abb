"""The Python shell of the sibling models (GRU4Rec, Caser, FEARec, LRURec, Mamba4Rec): what their kernel layers and
their model classes have in common, once.

  ``_KernelLayer``  a module whose forward and backward are one C call each: the workspace pool, the operand rule, the
                    evaluation-mode call and the ONE autograd node (``_LayerFn``).  ``FeaAttention`` is one without weights.
  ``_FlatLayer``    a ``_KernelLayer`` that owns ONE flat fp32 weight tensor whose slices are its parameters (``GruStack``,
                    ``CaserConv``, ``LruLayer``, ``MambaLayer``).
  ``_SiblingModel`` the models' plumbing: seed, generator and dropout, the device check, the catalogue head, the refusals.
  ``_BlockModel``   the body that LRURec and Mamba4Rec share: embedding, LayerNorm, N blocks of (layer, feed-forward), CE loss,
                    and the one-call training step of its "fused" mode (the flat weight array, the step buffers, the two calls).

A layer writes its parameter shapes, registration and initial values, ``_config`` and the two C calls (``_fwd`` / ``_bwd``); a
model writes its class attributes, its constructor, ``_encode`` (or its own ``forward`` / ``last_hidden``) and its loss."""
from __future__ import annotations

import math
from collections import OrderedDict

import torch
from torch import nn

from . import _fused_step as FS
from . import _lib as L
from .model import _CatalogueCeFn


def _no_cpu(how: str = "to the GPU"):
    return RuntimeError(f"bsarec_amd runs on MI355X only: move the model and its input {how} (there is no CPU fallback)")


def _operand(t):
    """What a kernel reads: detached, fp32, contiguous and 16-byte aligned (a clone when the view is not)."""
    t = t.detach().to(torch.float32).contiguous()
    return t.clone() if t.data_ptr() % 16 != 0 else t


def _layout(shapes, align: int = 1):
    """({name: (offset, numel, shape)}, total floats) of a flat array: every tensor starts at a multiple of ``align`` floats."""
    slices, off = OrderedDict(), 0
    for name, shp in shapes.items():
        off = (off + align - 1) // align * align
        n = math.prod(shp)
        slices[name] = (off, n, shp)
        off += n
    return slices, (off + align - 1) // align * align


class _LayerFn(torch.autograd.Function):
    """A kernel layer as one autograd node over its forward and backward C calls, both on the current stream.  ``tensors`` are
    the layer's inputs and behind them the views of its flat weight tensor (none for a layer without weights); ``extra`` is the
    layer's argument that is no tensor to differentiate (ids, last_only, the mode).  The workspace carries what the forward
    keeps to the backward: it is taken from the layer's pool and goes back after the backward.  The parameters' gradients are
    views of one flat ``dweights``."""

    @staticmethod
    def forward(ctx, layer, extra, *tensors):
        out, cfg, nbytes, key, ws, inputs = layer._run(tensors[:len(tensors) - len(layer._slices)], extra, True)
        ctx.save_for_backward(*inputs)
        ctx.layer, ctx.ws, ctx.call = layer, ws, (cfg, nbytes, key, extra, layer._flat)
        return out

    @staticmethod
    def backward(ctx, gout):
        inputs = ctx.saved_tensors
        cfg, nbytes, key, extra, flat = ctx.call
        layer = ctx.layer
        if ctx.ws is None:
            raise RuntimeError(f"{layer._tag}: backward ran twice (the forward's {layer._kept} are gone)")
        g = _operand(gout)
        grads = tuple(torch.empty_like(t) for t in inputs)
        dw = None if flat is None else torch.empty_like(flat)
        layer._bwd(cfg, inputs, extra, flat, g, ctx.ws, nbytes, grads, dw, torch.cuda.current_stream(g.device).cuda_stream)
        layer._pool[key].append(ctx.ws)
        ctx.ws = None
        return (None, None) + grads + tuple(dw[o:o + n].view(shp) for o, n, shp in layer._slices.values())


class _KernelLayer(nn.Module):
    """A subclass sets ``_tag`` (the word its messages start with) and ``_kept`` (what its workspace carries), and writes
      _config(inputs, extra, train) -> (cfg, nbytes)   its shape and device checks and its ``*_workspace_bytes`` call
      _fwd(cfg, inputs, extra, train, out, ws, nbytes, stream)                                the forward C call
      _bwd(cfg, inputs, extra, flat, g, ws, nbytes, grads, dweights, stream)                  the backward C call
      _out_shape(x, extra)                             when the output is not shaped like the first input
    and calls ``self._call(inputs, extra)`` from its ``forward``.  ``inputs`` is a tuple of [B, L, ...] tensors."""

    _tag, _kept = "", "activations"
    _slices, _flat = {}, None                    # a layer without weights (_FlatLayer has both)

    def __init__(self):
        super().__init__()
        self._pool = {}                          # (B, L, workspace bytes, device) -> free workspaces

    def flat_parameters(self):
        return []

    def _out_shape(self, x, extra):
        return x.shape

    def _run(self, inputs, extra, train: bool):
        """One forward call.  ``train``: the workspace is the backward's and stays out of the pool until that has run."""
        cfg, nbytes = self._config(inputs, extra, train)
        x = inputs[0]
        key = (x.shape[0], x.shape[1], nbytes, x.device)
        pool = self._pool.setdefault(key, [])
        ws = pool.pop() if pool else torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        inputs = tuple(_operand(t) for t in inputs)
        out = torch.empty(self._out_shape(inputs[0], extra), dtype=torch.float32, device=x.device)
        self._fwd(cfg, inputs, extra, int(train), out, ws, nbytes, torch.cuda.current_stream(x.device).cuda_stream)
        if not train:
            pool.append(ws)                      # stream order: the next user of ws runs after this call
        return out, cfg, nbytes, key, ws, inputs

    def _call(self, inputs, extra=None):
        """Differentiable with respect to the inputs and every parameter when autograd is recording; otherwise the train = 0
        call, which keeps nothing."""
        if not all(t.is_cuda for t in inputs):
            raise _no_cpu()
        params = self.flat_parameters()
        if params:
            self.reflatten()                     # once per call, before the views go anywhere
        if torch.is_grad_enabled() and (any(t.requires_grad for t in inputs) or any(p.requires_grad for p in params)):
            return _LayerFn.apply(self, extra, *inputs, *params)
        return self._run(inputs, extra, False)[0]


class _Holder(nn.Module):
    """Holder of a ``weight`` (and a ``bias``) that are views of a layer's flat tensor: the product runs in the layer's kernel."""

    def __init__(self, weight, bias=None):
        super().__init__()
        self.weight = weight
        if bias is not None:
            self.bias = bias


class _FlatLayer(_KernelLayer):
    """A kernel layer that owns ONE flat fp32 tensor ``_flat`` in the layout of its kernel's ``weights``; its parameters are views
    of it, so an optimiser that updates them in place updates the array the kernels read.  ``_make_flat(shapes, align)`` builds
    ``_slices`` {name: (offset, numel, shape)}, ``_numel``, ``_flat`` and the views as ``nn.Parameter``s in flat-array order, and
    returns them by name; the subclass registers them (the registration order is the state_dict's and is its own choice)."""

    def _make_flat(self, shapes, align: int = 1):
        self._slices, self._numel = _layout(shapes, align)
        self._flat = torch.zeros(self._numel, dtype=torch.float32)
        self._views = OrderedDict((name, nn.Parameter(self._flat[o:o + n].view(shp))) for name, (o, n, shp) in self._slices.items())
        return self._views

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        self.reflatten()
        return out

    def flat_parameters(self):
        """The parameters in the order of the flat array."""
        return list(self._views.values())

    def reflatten(self):
        """Makes every parameter a view of one flat tensor again (after ``.to()`` / ``.cuda()`` gave each its own storage).
        ``_flat`` may itself be a slice of a larger array (a ``_BlockModel`` in its fused mode): the test compares addresses,
        and ``data_ptr()`` of a slice is the address of its first element."""
        ps, base = self.flat_parameters(), self._flat
        if all(p.device == base.device and p.data_ptr() == base.data_ptr() + 4 * o
               for p, (o, n, shp) in zip(ps, self._slices.values())):
            return
        with torch.no_grad():
            flat = torch.zeros(self._numel, dtype=torch.float32, device=ps[0].device)
            for p, (o, n, shp) in zip(ps, self._slices.values()):
                flat[o:o + n] = p.detach().reshape(-1).to(torch.float32)
                p.data = flat[o:o + n].view(shp)
                p.grad = None
        self._flat, self._pool = flat, {}

    def _weights_on(self, x):
        """``_config``'s device check (``_call`` has made the flat tensor whole by now)."""
        if self._flat.device != x.device:
            raise RuntimeError(f"{self._tag}: the weights and the input are on different devices")

    def _scan_input(self, inputs, ids):
        """``_config``'s checks of a scan layer (LruLayer, MambaLayer) on x [B, L, width] and ids [B, L]; returns x."""
        (x,) = inputs
        if x.dim() != 3 or x.shape[2] != self.width:
            raise ValueError(f"{self._tag}: input must be [B, L, {self.width}], got {tuple(x.shape)}")
        if not x.is_cuda or (ids is not None and not ids.is_cuda):
            raise _no_cpu()
        if ids is not None and (tuple(ids.shape) != tuple(x.shape[:2]) or ids.dtype != torch.int64 or not ids.is_contiguous()):
            raise ValueError(f"{self._tag}: ids must be a contiguous int64 [B, L] = {tuple(x.shape[:2])}, got {tuple(ids.shape)} "
                             f"{ids.dtype}")
        self._weights_on(x)
        return x


class _LayerNorm(nn.Module):
    """TF-style LayerNorm, eps inside the square root, biased variance (the reference's, oracle/bsarec_oracle.py)."""

    def __init__(self, width: int, eps: float = 1e-12):
        super().__init__()
        self.weight, self.bias, self.eps = nn.Parameter(torch.ones(width)), nn.Parameter(torch.zeros(width)), eps

    def forward(self, x):
        u = x.mean(-1, keepdim=True)
        xc = x - u
        s = (xc * xc).mean(-1, keepdim=True)
        return self.weight * (xc / torch.sqrt(s + self.eps)) + self.bias


def _act(name: str):
    if name == "gelu":                                    # the erf form, as the reference writes it
        return lambda x: x * 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0)))
    return {"relu": torch.relu, "swish": lambda x: x * torch.sigmoid(x), "tanh": torch.tanh, "sigmoid": torch.sigmoid}[name]


class _FeedForward(nn.Module):
    def __init__(self, d: int):
        super().__init__()
        self.dense_1, self.dense_2 = nn.Linear(d, 4 * d), nn.Linear(4 * d, d)
        self.LayerNorm = _LayerNorm(d)


class _Encoder(nn.Module):
    def __init__(self, blocks):
        super().__init__()
        self.blocks = nn.ModuleList(blocks)


class _SiblingModel(nn.Module):
    """The plumbing of a sibling model.  The class attributes that Trainer reads (``needs_negatives``, ``torch_optim``,
    ``kernel_family``, ...) stay on the model; ``model_name`` is the name in its messages.  The model has ``item_embeddings`` and
    either ``_encode(input_ids, train)`` -> [x0, .. xN] or its own ``forward`` / ``last_hidden``."""

    model_name = ""

    def __init__(self, args):
        super().__init__()
        self.args = args
        self._seed, self._rank, self._gen = 42, 0, None
        self._fused = None                       # a fused step's buffers (the model's _step_buffers), where it has one
        self._ce_pool = {}                       # (B, V, d, device) -> free workspaces of bsarec_ce_head_*

    def _refuse_plan_options(self, args, own_loss: str):
        """The options of the plan models that a model with its own fp32 kernels and loss turns down at construction."""
        if getattr(args, "storage", None) == "bf16" or (getattr(args, "plan_options", None) or {}).get("storage", 0):
            raise ValueError(f"{self.model_name}: storage = 'bf16' does not apply (the {self.kernel_family} kernels are fp32)")
        if getattr(args, "train_negatives", 0):
            raise ValueError(f"{self.model_name}: train_negatives does not apply (the model has {own_loss})")
        if getattr(args, "train_lazy_adam", False):
            raise ValueError(f"{self.model_name}: train_lazy_adam does not apply (the model steps through torch.optim.Adam)")

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)         # every kernel layer has flattened itself again by now
        self._gen, self._ce_pool = None, {}
        self._fused = None                        # with the Adam moments and the step state, as the workspace pools go
        return out

    def check_trainer(self, args, process_group):
        """Called by Trainer before the first step."""
        if process_group is not None:
            raise ValueError(f"{self.model_name}: single GPU only")

    def _stream_seed(self):
        return (self._seed ^ (self._rank * 0x9E3779B97F4A7C15)) & 0x7FFFFFFFFFFFFFFF

    def set_seed(self, seed: int, rank: int = 0):
        """Seed of the dropout draws (rank-decorrelated): of the torch generator and, where the model has a fused step, of its
        device state, whose step counter goes back to 0."""
        self._seed, self._rank, self._gen = int(seed), int(rank), None
        if self._fused is not None:
            self._fused["state"][0] = self._stream_seed()
            self._fused["state"][1] = 0

    def _generator(self, device):
        if self._gen is None or self._gen.device != device:
            self._gen = torch.Generator(device=device)
            self._gen.manual_seed(self._stream_seed())
        return self._gen

    def _drop(self, x, p: float, train: bool):
        if not train or p <= 0.0:
            return x
        keep = torch.empty_like(x).bernoulli_(1.0 - p, generator=self._generator(x.device))
        return x * keep * (1.0 / (1.0 - p))

    def _require_gpu(self, input_ids=None):
        if self.item_embeddings.weight.device.type != "cuda" or (input_ids is not None and not input_ids.is_cuda):
            raise _no_cpu("with .cuda()")
        if input_ids is not None:
            self._check_ids(input_ids)

    def _check_ids(self, input_ids):
        """The model's own shape rule (Caser and FEARec pin L)."""
        if input_ids.dim() != 2:
            raise ValueError(f"{self.model_name}: input_ids must be [B, L], got {tuple(input_ids.shape)}")

    def forward(self, input_ids, user_ids=None, all_sequence_output=False):
        """[B, L] ids -> the last block's [B, L, d], or every layer's outputs as a list.  ``user_ids`` is ignored."""
        self._require_gpu(input_ids)
        outs = self._encode(input_ids, self.training)
        return outs if all_sequence_output else outs[-1]

    def predict(self, input_ids, user_ids=None, all_sequence_output=False):
        return self.forward(input_ids, user_ids, all_sequence_output)

    def last_hidden(self, input_ids) -> torch.Tensor:
        """[B, d]: position L - 1 of the evaluation-mode output (no dropout), no gradient."""
        self._require_gpu(input_ids)
        with torch.no_grad():
            return self._encode(input_ids, False)[-1][:, -1, :]

    def catalogue_weight(self) -> torch.Tensor:
        return self.item_embeddings.weight.detach()

    def catalogue_ce(self, seq_output, answers) -> torch.Tensor:
        """``F.cross_entropy(seq_output @ E.T, answers)`` as one HIP autograd node (bsarec_ce_head_fwd / _bwd)."""
        return _CatalogueCeFn.apply(self, seq_output, self.item_embeddings.weight, answers)

    @property
    def step_state(self) -> torch.Tensor:
        """The fused step's device state, int64[8]: [0] the Philox seed, [1] the step counter of the dropout stream, [2] Adam's t."""
        return self._step_buffers()["state"]

    def _torch_steps(self, tail: str = " (Trainer does)"):
        return RuntimeError(f"{self.model_name} steps through calculate_loss / backward / torch.optim.Adam{tail}")

    def train_step(self, input_ids, answers, neg_answers=None, same_target=None):
        raise self._torch_steps()

    def grad_step(self, input_ids, answers, neg_answers=None):
        raise self._torch_steps()


class _Block(nn.Module):
    """``item_encoder.blocks.{k}``: the kernel layer under the model's name for it, with the LayerNorm behind its residual as the
    layer's own child, and the feed-forward net."""

    def __init__(self, name: str, layer: nn.Module, d: int):
        super().__init__()
        layer.LayerNorm = _LayerNorm(d)
        setattr(self, name, layer)
        self.feed_forward = _FeedForward(d)


class _BlockModel(_SiblingModel):
    """x = Dropout(LN(E[ids])); per block: z = layer(x, ids); a = LN(Dropout(z) + x); x = LN(Dropout(dense_2(gelu(dense_1(a)))) + a);
    the loss is the full-catalogue cross-entropy of the last position.  ``layer_attr`` names the layer inside a block (the
    state_dict keys), ``make_layer(d, std)`` builds one.

    ``args.<step_flag>`` ("torch", the default, or "fused") selects how the model steps; the mode is kept under the flag's name
    (``model.lru_step``, ``model.mamba_step``).  In the fused mode ``train_step`` is ONE C call, the model owns ONE flat fp32
    tensor in the layout of that call's ``weights``, every parameter but the item table is a view of it and each layer's
    ``_flat`` a slice of it, and the instance sets ``torch_optim = False`` and ``own_train_step = True``.  A model supplies
      step_flag                    the flag's name; ``args.<step_flag>_graph = False`` steps eagerly instead of replaying a graph
      step_calls                   the prefix of its three C calls: ``<prefix>_workspace_bytes``, ``_loss_grad``, ``_train_step``
      _param_shapes()              its ``*_param_shapes(width, layers, ...)``: the flat array under the state_dict keys
      _step_config(B, L)           the config struct of the three calls"""

    layer_attr = ""
    step_flag = ""
    step_calls = ""

    def __init__(self, args, make_layer):
        mode = getattr(args, self.step_flag, "torch")
        if mode not in ("torch", "fused"):
            raise ValueError(f"{self.step_flag} must be 'torch' or 'fused', got {mode!r}")
        super().__init__(args)
        self._refuse_plan_options(args, "the full-catalogue cross-entropy")
        d, N = int(args.hidden_size), int(args.num_hidden_layers)
        if N < 1:
            raise ValueError(f"{self.model_name}: num_hidden_layers = {N}, expected N >= 1")
        self.p_hidden = float(args.hidden_dropout_prob)
        if not 0.0 <= self.p_hidden < 1.0:
            raise ValueError(f"dropout probabilities must be in [0, 1), got {self.p_hidden}")
        self._actf = _act("gelu")
        std = float(args.initializer_range)
        self.item_embeddings = nn.Embedding(int(args.item_size), d)
        self.LayerNorm = _LayerNorm(d)
        self.item_encoder = _Encoder(_Block(self.layer_attr, make_layer(d, std), d) for _ in range(N))
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, (nn.Linear, nn.Embedding)):
                    m.weight.normal_(0.0, std)
                if isinstance(m, nn.Linear):
                    m.bias.zero_()
        setattr(self, self.step_flag, mode)
        if mode == "fused":
            self.torch_optim, self.own_train_step = False, True
        self._wflat = None                       # the fused mode: the flat weight array (reflatten)
        self._wslices, _ = _layout(self._param_shapes())       # state_dict key -> (offset, floats, shape) in the flat array
        self.reflatten()

    def _is_fused(self) -> bool:
        return getattr(self, self.step_flag) == "fused"

    def _layers(self):
        return [getattr(blk, self.layer_attr) for blk in self.item_encoder.blocks]

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)         # every layer has flattened itself again by now
        self.reflatten()
        return out

    def flat_parameters(self):
        """Every parameter but the item table, in the order of the flat weight array."""
        named = dict(self.named_parameters())
        return [named[k] for k in self._wslices]

    def reflatten(self):
        """The fused mode: makes every parameter but the item table a view of ONE flat tensor in the layout of the step's
        ``weights`` and every layer's ``_flat`` a slice of it (at construction, and after ``.to()`` / ``.cuda()`` gave the
        parameters storages of their own and the layers flattened themselves).  The values do not change.  A no-op in the
        default mode."""
        if not self._is_fused():
            return
        ps, base = self.flat_parameters(), self._wflat
        if base is not None and all(p.device == base.device and p.data_ptr() == base.data_ptr() + 4 * o
                                    for p, (o, n, shp) in zip(ps, self._wslices.values())):
            return
        with torch.no_grad():
            flat = torch.cat([p.detach().reshape(-1).to(torch.float32) for p in ps])
            for p, (o, n, shp) in zip(ps, self._wslices.values()):
                p.data = flat[o:o + n].view(shp)
                p.grad = None
        self._wflat, self._fused = flat, None
        for k, layer in enumerate(self._layers()):
            o = self._wslices[f"item_encoder.blocks.{k}.{self.layer_attr}.{next(iter(layer._slices))}"][0]
            layer._flat, layer._pool = flat[o:o + layer._numel], {}

    def _encode(self, input_ids, train: bool):
        """Every layer's output, [x0, x1, .. xN]."""
        ids = input_ids.to(torch.int64).contiguous()
        p = self.p_hidden
        x = self._drop(self.LayerNorm(self.item_embeddings(ids)), p, train)
        outs = [x]
        for blk in self.item_encoder.blocks:
            layer, ff = getattr(blk, self.layer_attr), blk.feed_forward
            a = layer.LayerNorm(self._drop(layer(x, ids), p, train) + x)
            x = ff.LayerNorm(self._drop(ff.dense_2(self._actf(ff.dense_1(a))), p, train) + a)
            outs.append(x)
        return outs

    def calculate_loss(self, input_ids, answers, neg_answers=None, same_target=None, user_ids=None):
        """The full-catalogue cross-entropy of the last position: a 0-d tensor."""
        self._require_gpu(input_ids)
        return self.catalogue_ce(self.forward(input_ids)[:, -1, :], answers)

    # ---- the fused step (<step_calls>_loss_grad / _train_step; host side: _fused_step.py) ----
    def _step_buffers(self):
        """What the fused step owns beside the parameters: the device step state (seed, step counter, Adam t), both gradient
        arrays, the Adam moments of the item table ("E") and of the flat weight array ("W"), and per batch shape a workspace,
        static id buffers and a captured graph.  Built on first use; dropped by ``.to()`` / ``reflatten()`` (a new parameter
        storage)."""
        if not self._is_fused():
            raise self._torch_steps(f" (Trainer does); the one-call step needs {self.step_flag} = 'fused'")
        self._require_gpu()
        self.reflatten()
        E, flat = self.item_embeddings.weight.data, self._wflat
        if flat.device != E.device or not E.is_contiguous() or E.dtype != torch.float32:
            raise RuntimeError(f"{self.model_name.lower()}: the item table and the flat weight array must be contiguous fp32 on "
                               f"one device")
        self._fused = FS.buffers(self._fused, [("E", E), ("W", flat)], self._stream_seed())
        return self._fused

    def _slot(self, f, B: int, Lq: int):
        s = f["slots"].get((B, Lq))
        if s is None:
            cfg = self._step_config(B, Lq)
            nbytes = getattr(L.load(), self.step_calls + "_workspace_bytes")(cfg)
            if nbytes < 0:
                raise ValueError(f"{self.model_name.lower()}: unsupported step shape B = {B}, L = {Lq}, N = {cfg.layers}, "
                                 f"dropout = {self.p_hidden} (1 <= B <= 65536, 1 <= L <= 256, 1 <= N <= {L.MAX_LAYERS}, "
                                 f"0 <= p < 1)")
            s = FS.slot(f, (B, Lq), cfg, nbytes, (B, Lq))           # the slot's ``neg`` buffer stays unused
        return s

    def _fill(self, s, input_ids, answers):
        self._require_gpu(input_ids)
        s["ids"].copy_(input_ids)
        s["ans"].copy_(answers.reshape(-1))
        return s

    def _loss_grad(self, f, s, train: bool):
        name = self.step_calls + "_loss_grad"
        L.check(getattr(L.load(), name)(s["cfg"], f["E"].data_ptr(), f["W"].data_ptr(), s["ids"].data_ptr(), s["ans"].data_ptr(),
                                        f["state"].data_ptr(), int(train), s["loss"].data_ptr(), f["dE"].data_ptr(),
                                        f["dW"].data_ptr(), s["ws"].data_ptr(), s["nbytes"], FS.stream(f)), name)

    def loss_and_grads(self, input_ids, answers, train: bool = False):
        """The loss (0-d tensor) and {state_dict key: gradient} of one batch through the step's ``_loss_grad`` call, no update.
        ``train``: draw the next dropout masks of the device stream (the step counter advances); else no dropout."""
        f = self._step_buffers()
        s = self._fill(self._slot(f, int(input_ids.shape[0]), int(input_ids.shape[1])), input_ids, answers)
        self._loss_grad(f, s, train)
        grads = OrderedDict([("item_embeddings.weight", f["dE"].clone())])
        for name, (o, n, shp) in self._wslices.items():
            grads[name] = f["dW"][o:o + n].view(shp).clone()
        return s["loss"].clone(), grads

    def _train_step(self, f, s):
        items, weights = FS.adam_structs(f, self.args)
        name = self.step_calls + "_train_step"
        L.check(getattr(L.load(), name)(s["cfg"], s["ids"].data_ptr(), s["ans"].data_ptr(), items, weights, f["state"].data_ptr(),
                                        s["loss"].data_ptr(), s["ws"].data_ptr(), s["nbytes"], FS.stream(f)), name)

    def train_step(self, input_ids, answers, neg_answers=None, same_target=None):
        """The fused mode: one optimisation step in one C call -- the step counter, lookup + LayerNorm + Philox dropout, the
        blocks, the CE head, every gradient, Adam (``args.lr``, ``adam_beta1``, ``adam_beta2``, ``weight_decay``) on the item
        table and on the flat weight array, in place.  Returns the mean loss as a 0-d device tensor (no host sync; the next step
        overwrites it).  The call is captured once per batch shape over static id buffers and replayed -- the masks and Adam's t
        advance on the device, and the capture is one linear chain on one stream, so it has no parallel branches to replay;
        ``args.<step_flag>_graph = False`` calls eagerly instead.  ``neg_answers`` and ``same_target`` are ignored."""
        if not self._is_fused():
            raise self._torch_steps()
        f = self._step_buffers()
        s = self._fill(self._slot(f, int(input_ids.shape[0]), int(input_ids.shape[1])), input_ids, answers)
        return FS.train_step(f, s, self.args, getattr(self.args, self.step_flag + "_graph", True), self._loss_grad,
                             self._train_step)
