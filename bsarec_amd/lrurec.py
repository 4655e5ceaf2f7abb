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
(bsarec_ce_head_fwd / _bwd); the embedding lookup, the LayerNorms, the feed-forward net and the dropout are torch ops.  There
is no CPU path.
"""
from __future__ import annotations

import math
from collections import OrderedDict

import torch
from torch import nn

from . import _lib as L
from .fearec import _LayerNorm, _act
from .model import _CatalogueCeFn

_NO_CPU = "bsarec_amd runs on MI355X only: move the model and its input to the GPU (there is no CPU fallback)"


def lru_param_shapes(width: int) -> "OrderedDict[str, tuple]":
    """The tensors of bsarec_lru_fwd's flat weight array, in its order (include/bsarec_hip.h)."""
    d = int(width)
    return OrderedDict([("nu_log", (d,)), ("theta_log", (d,)), ("gamma_log", (d,)), ("in_proj.weight", (2 * d, d)),
                        ("in_proj.bias", (2 * d,)), ("out_proj.weight", (d, 2 * d)), ("out_proj.bias", (d,))])


class _LruFn(torch.autograd.Function):
    """The layer as one autograd node over bsarec_lru_fwd / bsarec_lru_bwd, both on the current stream.  The workspace carries
    v and h to the backward: it is taken from the layer's pool per shape and goes back after the backward.  ``params`` are the
    views of the layer's flat weight tensor; their gradients are views of one flat ``dweights``."""

    @staticmethod
    def forward(ctx, layer, x, ids, *params):
        cfg, nbytes = layer._config(x, ids, 1)
        key = (x.shape[0], x.shape[1], True, x.device)
        pool = layer._pool.setdefault(key, [])
        ws = pool.pop() if pool else torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        x = layer._operand(x)
        y = torch.empty_like(x)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        L.check(L.load().bsarec_lru_fwd(cfg, x.data_ptr(), None if ids is None else ids.data_ptr(), layer._flat.data_ptr(), 1,
                                        y.data_ptr(), ws.data_ptr(), nbytes, stream), "bsarec_lru_fwd")
        ctx.save_for_backward(x)
        ctx.layer, ctx.key, ctx.ws, ctx.call = layer, key, ws, (cfg, nbytes, ids, layer._flat)
        return y

    @staticmethod
    def backward(ctx, gout):
        (x,) = ctx.saved_tensors
        cfg, nbytes, ids, flat = ctx.call
        layer = ctx.layer
        if ctx.ws is None:
            raise RuntimeError("lru: backward ran twice (the forward's activations are gone)")
        g = layer._operand(gout)
        dx = torch.empty_like(x)
        dw = torch.empty_like(flat)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        L.check(L.load().bsarec_lru_bwd(cfg, x.data_ptr(), None if ids is None else ids.data_ptr(), flat.data_ptr(), g.data_ptr(),
                                        ctx.ws.data_ptr(), nbytes, dx.data_ptr(), dw.data_ptr(), stream), "bsarec_lru_bwd")
        layer._pool[ctx.key].append(ctx.ws)
        ctx.ws = None
        return (None, dx, None) + tuple(dw[o:o + n].view(shp) for o, n, shp in layer._slices.values())


class _Proj(nn.Module):
    """Holder of ``in_proj`` / ``out_proj``: views of the layer's flat tensor (the products run in bsarec_lru_fwd)."""

    def __init__(self, weight, bias):
        super().__init__()
        self.weight, self.bias = weight, bias


class LruLayer(nn.Module):
    """x [B, L, d], ids [B, L] (0 is padding; ``None``: no padding) -> y [B, L, d] on the HIP kernels, with m_t = (ids_t != 0):
      lambda = exp(-exp(nu_log)) (cos(exp(theta_log)) + i sin(exp(theta_log)))                       |lambda| < 1 always
      u_t = in_proj(x_t) (first d entries real, last d imaginary);  v_t = m_t exp(gamma_log) u_t
      h_t = lambda h_{t-1} + v_t, h_{-1} = 0;   y_t = out_proj([Re h_t | Im h_t])
    Owns ONE flat fp32 tensor in the layout of bsarec_lru_fwd's ``weights``; ``nu_log``, ``theta_log``, ``gamma_log``,
    ``in_proj.{weight,bias}`` and ``out_proj.{weight,bias}`` are parameters that are views of it, so an optimiser that updates them
    in place updates the array the kernels read.

    Init: u1, u2 ~ U(0, 1) per channel, nu_log = log(-1/2 log(u1 (r_max^2 - r_min^2) + r_min^2)), theta_log = log(2 pi u2),
    gamma_log = log sqrt(1 - |lambda|^2), which puts |lambda| in [r_min, r_max]; projection weights N(0, ``std``), biases 0."""

    def __init__(self, width: int, r_min: float = 0.8, r_max: float = 0.99, std: float = 0.02):
        super().__init__()
        d = int(width)
        if not (4 <= d <= 256 and d % 4 == 0):
            raise ValueError(f"LRURec: hidden_size {d} outside 4..256 or not a multiple of 4")
        if not 0.0 <= r_min < r_max < 1.0:
            raise ValueError(f"LRURec: lru_r_min = {r_min}, lru_r_max = {r_max}: expected 0 <= r_min < r_max < 1")
        self.width, self.r_min, self.r_max = d, float(r_min), float(r_max)
        self._slices = OrderedDict()
        off = 0
        for name, shp in lru_param_shapes(d).items():
            n = math.prod(shp)
            self._slices[name] = (off, n, shp)
            off += n
        self._pool = {}                          # (B, L, train, device) -> free workspaces
        self._flat = torch.zeros(off, dtype=torch.float32)
        self._views = OrderedDict()
        for name, (o, n, shp) in self._slices.items():
            self._views[name] = nn.Parameter(self._flat[o:o + n].view(shp))
        v = self._views
        for name in ("nu_log", "theta_log", "gamma_log"):
            self.register_parameter(name, v[name])
        self.in_proj = _Proj(v["in_proj.weight"], v["in_proj.bias"])
        self.out_proj = _Proj(v["out_proj.weight"], v["out_proj.bias"])
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

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        self.reflatten()
        return out

    def flat_parameters(self):
        """The parameters in the order of the flat array."""
        return list(self._views.values())

    def reflatten(self):
        """Makes every parameter a view of one flat tensor again (after ``.to()`` / ``.cuda()`` gave each its own storage)."""
        ps = self.flat_parameters()
        base = self._flat
        if all(p.device == base.device and p.data_ptr() == base.data_ptr() + 4 * o
               for p, (o, n, shp) in zip(ps, self._slices.values())):
            return
        with torch.no_grad():
            flat = torch.cat([p.detach().reshape(-1).to(torch.float32) for p in ps])
            for p, (o, n, shp) in zip(ps, self._slices.values()):
                p.data = flat[o:o + n].view(shp)
                p.grad = None
        self._flat = flat
        self._pool = {}

    def _config(self, x, ids, train):
        if x.dim() != 3 or x.shape[2] != self.width:
            raise ValueError(f"lru: input must be [B, L, {self.width}], got {tuple(x.shape)}")
        if not x.is_cuda or (ids is not None and not ids.is_cuda):
            raise RuntimeError(_NO_CPU)
        if ids is not None and (tuple(ids.shape) != tuple(x.shape[:2]) or ids.dtype != torch.int64 or not ids.is_contiguous()):
            raise ValueError(f"lru: ids must be a contiguous int64 [B, L] = {tuple(x.shape[:2])}, got {tuple(ids.shape)} {ids.dtype}")
        self.reflatten()
        if self._flat.device != x.device:
            raise RuntimeError("lru: the weights and the input are on different devices")
        cfg = L.LruConfig(x.shape[0], x.shape[1], self.width)
        nbytes = L.load().bsarec_lru_workspace_bytes(cfg, int(train))
        if nbytes < 0:
            raise ValueError(f"lru: unsupported shape B = {x.shape[0]}, L = {x.shape[1]} (1 <= B <= 65536, 1 <= L <= 256)")
        return cfg, nbytes

    @staticmethod
    def _operand(t):
        t = t.detach().to(torch.float32).contiguous()
        return t.clone() if t.data_ptr() % 16 != 0 else t

    def forward(self, x, ids=None):
        """Differentiable with respect to x and every parameter when autograd is recording; otherwise the train = 0 call,
        which keeps nothing."""
        if not x.is_cuda:
            raise RuntimeError(_NO_CPU)
        if ids is not None:
            ids = ids.to(torch.int64).contiguous()
        params = self.flat_parameters()
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params)):
            self.reflatten()
            return _LruFn.apply(self, x, ids, *params)
        cfg, nbytes = self._config(x, ids, 0)
        key = (x.shape[0], x.shape[1], False, x.device)
        pool = self._pool.setdefault(key, [])
        ws = pool.pop() if pool else torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        xo = self._operand(x)
        y = torch.empty_like(xo)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        L.check(L.load().bsarec_lru_fwd(cfg, xo.data_ptr(), None if ids is None else ids.data_ptr(), self._flat.data_ptr(), 0,
                                        y.data_ptr(), ws.data_ptr(), nbytes, stream), "bsarec_lru_fwd")
        pool.append(ws)                          # stream order: the next user of ws runs after this call
        return y


class _LruBlockLayer(LruLayer):
    """``item_encoder.blocks.{k}.lru``: the recurrent layer and the LayerNorm behind its residual."""

    def __init__(self, width, r_min, r_max, std):
        super().__init__(width, r_min, r_max, std)
        self.LayerNorm = _LayerNorm(width)


class _FeedForward(nn.Module):
    def __init__(self, d: int):
        super().__init__()
        self.dense_1, self.dense_2 = nn.Linear(d, 4 * d), nn.Linear(4 * d, d)
        self.LayerNorm = _LayerNorm(d)


class _Block(nn.Module):
    def __init__(self, d, r_min, r_max, std):
        super().__init__()
        self.lru = _LruBlockLayer(d, r_min, r_max, std)
        self.feed_forward = _FeedForward(d)


class _Encoder(nn.Module):
    def __init__(self, blocks):
        super().__init__()
        self.blocks = nn.ModuleList(blocks)


class LRURecModel(nn.Module):
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
    ``LruLayer`` has them with ``lru_r_min`` (default 0.8) and ``lru_r_max`` (default 0.99)."""

    needs_negatives = False
    needs_same_target = False
    torch_optim = True
    full_logits = None                           # no dense-logits path: the rankings take last_hidden + catalogue_weight
    kernel_family = "LRU"

    def __init__(self, args):
        super().__init__()
        if getattr(args, "storage", None) == "bf16" or (getattr(args, "plan_options", None) or {}).get("storage", 0):
            raise ValueError("LRURec: storage = 'bf16' does not apply (the LRU kernels are fp32)")
        if getattr(args, "train_negatives", 0):
            raise ValueError("LRURec: train_negatives does not apply (the model has the full-catalogue cross-entropy)")
        if getattr(args, "train_lazy_adam", False):
            raise ValueError("LRURec: train_lazy_adam does not apply (the model steps through torch.optim.Adam)")
        self.args = args
        d, N = int(args.hidden_size), int(args.num_hidden_layers)
        if N < 1:
            raise ValueError(f"LRURec: num_hidden_layers = {N}, expected N >= 1")
        r_min, r_max = float(getattr(args, "lru_r_min", 0.8)), float(getattr(args, "lru_r_max", 0.99))
        self.p_hidden = float(args.hidden_dropout_prob)
        if not 0.0 <= self.p_hidden < 1.0:
            raise ValueError(f"dropout probabilities must be in [0, 1), got {self.p_hidden}")
        self._actf = _act("gelu")
        std = float(args.initializer_range)
        self.item_embeddings = nn.Embedding(int(args.item_size), d)
        self.LayerNorm = _LayerNorm(d)
        self.item_encoder = _Encoder(_Block(d, r_min, r_max, std) for _ in range(N))
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, (nn.Linear, nn.Embedding)):
                    m.weight.normal_(0.0, std)
                if isinstance(m, nn.Linear):
                    m.bias.zero_()
        self._ce_pool = {}                       # (B, V, d, device) -> free workspaces of bsarec_ce_head_*
        self._seed, self._rank, self._gen = 42, 0, None

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        self._gen, self._ce_pool = None, {}
        return out

    def check_trainer(self, args, process_group):
        """Called by Trainer before the first step."""
        if process_group is not None:
            raise ValueError("LRURec: single GPU only")

    def set_seed(self, seed: int, rank: int = 0):
        """Seed of the dropout draws (rank-decorrelated)."""
        self._seed, self._rank, self._gen = int(seed), int(rank), None

    def _generator(self, device):
        if self._gen is None or self._gen.device != device:
            self._gen = torch.Generator(device=device)
            self._gen.manual_seed((self._seed ^ (self._rank * 0x9E3779B97F4A7C15)) & 0x7FFFFFFFFFFFFFFF)
        return self._gen

    def _drop(self, x, train):
        p = self.p_hidden
        if not train or p <= 0.0:
            return x
        keep = torch.empty_like(x).bernoulli_(1.0 - p, generator=self._generator(x.device))
        return x * keep * (1.0 / (1.0 - p))

    def _require_gpu(self, input_ids=None):
        if self.item_embeddings.weight.device.type != "cuda" or (input_ids is not None and not input_ids.is_cuda):
            raise RuntimeError("bsarec_amd runs on MI355X only: move the model and its input with .cuda() "
                               "(there is no CPU fallback)")
        if input_ids is not None and input_ids.dim() != 2:
            raise ValueError(f"LRURec: input_ids must be [B, L], got {tuple(input_ids.shape)}")

    def _encode(self, input_ids, train: bool):
        """Every layer's output, [x0, x1, .. xN]."""
        ids = input_ids.to(torch.int64).contiguous()
        x = self._drop(self.LayerNorm(self.item_embeddings(ids)), train)
        outs = [x]
        for blk in self.item_encoder.blocks:
            ff = blk.feed_forward
            a = blk.lru.LayerNorm(self._drop(blk.lru(x, ids), train) + x)
            x = ff.LayerNorm(self._drop(ff.dense_2(self._actf(ff.dense_1(a))), train) + a)
            outs.append(x)
        return outs

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

    def calculate_loss(self, input_ids, answers, neg_answers=None, same_target=None, user_ids=None):
        """The full-catalogue cross-entropy of the last position: a 0-d tensor."""
        self._require_gpu(input_ids)
        return self.catalogue_ce(self.forward(input_ids)[:, -1, :], answers)

    def train_step(self, input_ids, answers, neg_answers=None, same_target=None):
        raise RuntimeError("LRURec steps through calculate_loss / backward / torch.optim.Adam (Trainer does)")

    def grad_step(self, input_ids, answers, neg_answers=None):
        raise RuntimeError("LRURec steps through calculate_loss / backward / torch.optim.Adam (Trainer does)")
