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
from .lrurec import _FeedForward
from .model import _CatalogueCeFn

_NO_CPU = "bsarec_amd runs on MI355X only: move the model and its input to the GPU (there is no CPU fallback)"


def default_dt_rank(width: int) -> int:
    """``--mamba_dt_rank`` when absent: 4 ceil(d / 64)."""
    return 4 * math.ceil(int(width) / 64)


def mamba_param_shapes(width: int, expand: int, d_state: int, d_conv: int, dt_rank: int) -> "OrderedDict[str, tuple]":
    """The tensors of bsarec_mamba_fwd's flat weight array, in its order (include/bsarec_hip.h)."""
    d, di, N, K, R = int(width), int(expand) * int(width), int(d_state), int(d_conv), int(dt_rank)
    return OrderedDict([("in_proj.weight", (2 * di, d)), ("conv1d.weight", (di, K)), ("conv1d.bias", (di,)),
                        ("x_proj.weight", (R + 2 * N, di)), ("dt_proj.weight", (di, R)), ("dt_proj.bias", (di,)),
                        ("A_log", (di, N)), ("D", (di,)), ("out_proj.weight", (d, di))])


class _MambaFn(torch.autograd.Function):
    """The layer as one autograd node over bsarec_mamba_fwd / bsarec_mamba_bwd, both on the current stream.  The workspace
    carries the activations and the state checkpoints to the backward: it is taken from the layer's pool per shape and goes back
    after the backward.  ``params`` are the views of the layer's flat weight tensor; their gradients are views of one flat
    ``dweights``."""

    @staticmethod
    def forward(ctx, layer, x, ids, *params):
        cfg, nbytes = layer._config(x, ids, 1)
        key = (x.shape[0], x.shape[1], True, x.device)
        pool = layer._pool.setdefault(key, [])
        ws = pool.pop() if pool else torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        x = layer._operand(x)
        out = torch.empty_like(x)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        L.check(L.load().bsarec_mamba_fwd(cfg, x.data_ptr(), None if ids is None else ids.data_ptr(), layer._flat.data_ptr(), 1,
                                          out.data_ptr(), ws.data_ptr(), nbytes, stream), "bsarec_mamba_fwd")
        ctx.save_for_backward(x)
        ctx.layer, ctx.key, ctx.ws, ctx.call = layer, key, ws, (cfg, nbytes, ids, layer._flat)
        return out

    @staticmethod
    def backward(ctx, gout):
        (x,) = ctx.saved_tensors
        cfg, nbytes, ids, flat = ctx.call
        layer = ctx.layer
        if ctx.ws is None:
            raise RuntimeError("mamba: backward ran twice (the forward's activations are gone)")
        g = layer._operand(gout)
        dx = torch.empty_like(x)
        dw = torch.empty_like(flat)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        L.check(L.load().bsarec_mamba_bwd(cfg, x.data_ptr(), None if ids is None else ids.data_ptr(), flat.data_ptr(), g.data_ptr(),
                                          ctx.ws.data_ptr(), nbytes, dx.data_ptr(), dw.data_ptr(), stream), "bsarec_mamba_bwd")
        layer._pool[ctx.key].append(ctx.ws)
        ctx.ws = None
        return (None, dx, None) + tuple(dw[o:o + n].view(shp) for o, n, shp in layer._slices.values())


class _Holder(nn.Module):
    """Holder of ``in_proj`` / ``conv1d`` / ``x_proj`` / ``dt_proj`` / ``out_proj``: views of the layer's flat tensor (the
    products and the convolution run in bsarec_mamba_fwd)."""

    def __init__(self, weight, bias=None):
        super().__init__()
        self.weight = weight
        if bias is not None:
            self.bias = bias


class MambaLayer(nn.Module):
    """x [B, L, d], ids [B, L] (0 is padding; ``None``: no padding) -> out [B, L, d] on the HIP kernels, with d_inner = expand d,
    N = d_state, K = d_conv, R = dt_rank and m_t = (ids_t != 0):
      [xs_t | z_t] = in_proj(x_t);  c_t[j] = conv1d.bias[j] + sum_{k<K} conv1d.weight[j, k] (m_s xs_s[j]), s = t - K + 1 + k >= 0
      u_t = silu(c_t);  [delta_t | B_t | C_t] = x_proj(u_t);  Delta_t = softplus(dt_proj(delta_t));  A = -exp(A_log)
      m_t: h_t[j, n] = exp(Delta_t[j] A[j, n]) h_{t-1}[j, n] + Delta_t[j] B_t[n] u_t[j];  else h_t = h_{t-1};  h_{-1} = 0
      s_t[j] = sum_n C_t[n] h_t[j, n] + D[j] u_t[j];  y_t = m_t ? s_t silu(z_t) : 0;  out_t = out_proj(y_t)
    Owns ONE flat fp32 tensor in the layout of bsarec_mamba_fwd's ``weights``; ``in_proj.weight``, ``conv1d.{weight,bias}``,
    ``x_proj.weight``, ``dt_proj.{weight,bias}``, ``A_log``, ``D`` and ``out_proj.weight`` are parameters that are views of it, so
    an optimiser that updates them in place updates the array the kernels read.  ``conv1d.weight`` is [d_inner, K] (torch's
    depthwise Conv1d weight without its middle axis of 1).

    Init: Linear weights N(0, ``std``), conv1d weight and bias U(+-K^-1/2), dt_proj.weight U(+-R^-1/2), dt_proj.bias =
    softplus^-1(dt) with dt log-uniform in [1e-3, 1e-1], A_log[j, n] = log(n + 1), D = 1."""

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
        self._slices = OrderedDict()
        off = 0
        for name, shp in mamba_param_shapes(d, E, N, K, R).items():
            n = math.prod(shp)
            self._slices[name] = (off, n, shp)
            off += n
        self._pool = {}                          # (B, L, train, device) -> free workspaces
        self._flat = torch.zeros(off, dtype=torch.float32)
        self._views = OrderedDict()
        for name, (o, n, shp) in self._slices.items():
            self._views[name] = nn.Parameter(self._flat[o:o + n].view(shp))
        v = self._views
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
            raise ValueError(f"mamba: input must be [B, L, {self.width}], got {tuple(x.shape)}")
        if not x.is_cuda or (ids is not None and not ids.is_cuda):
            raise RuntimeError(_NO_CPU)
        if ids is not None and (tuple(ids.shape) != tuple(x.shape[:2]) or ids.dtype != torch.int64 or not ids.is_contiguous()):
            raise ValueError(f"mamba: ids must be a contiguous int64 [B, L] = {tuple(x.shape[:2])}, got {tuple(ids.shape)} {ids.dtype}")
        self.reflatten()
        if self._flat.device != x.device:
            raise RuntimeError("mamba: the weights and the input are on different devices")
        cfg = L.MambaConfig(x.shape[0], x.shape[1], self.width, self.expand, self.d_state, self.d_conv, self.dt_rank)
        nbytes = L.load().bsarec_mamba_workspace_bytes(cfg, int(train))
        if nbytes < 0:
            raise ValueError(f"mamba: unsupported shape B = {x.shape[0]}, L = {x.shape[1]} (1 <= B <= 65536, 1 <= L <= 256)")
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
            return _MambaFn.apply(self, x, ids, *params)
        cfg, nbytes = self._config(x, ids, 0)
        key = (x.shape[0], x.shape[1], False, x.device)
        pool = self._pool.setdefault(key, [])
        ws = pool.pop() if pool else torch.empty(nbytes, dtype=torch.uint8, device=x.device)
        xo = self._operand(x)
        out = torch.empty_like(xo)
        stream = torch.cuda.current_stream(x.device).cuda_stream
        L.check(L.load().bsarec_mamba_fwd(cfg, xo.data_ptr(), None if ids is None else ids.data_ptr(), self._flat.data_ptr(), 0,
                                          out.data_ptr(), ws.data_ptr(), nbytes, stream), "bsarec_mamba_fwd")
        pool.append(ws)                          # stream order: the next user of ws runs after this call
        return out


class _MambaBlockLayer(MambaLayer):
    """``item_encoder.blocks.{k}.mamba``: the state-space layer and the LayerNorm behind its residual."""

    def __init__(self, width, d_state, d_conv, expand, dt_rank, std):
        super().__init__(width, d_state, d_conv, expand, dt_rank, std)
        self.LayerNorm = _LayerNorm(width)


class _Block(nn.Module):
    def __init__(self, d, d_state, d_conv, expand, dt_rank, std):
        super().__init__()
        self.mamba = _MambaBlockLayer(d, d_state, d_conv, expand, dt_rank, std)
        self.feed_forward = _FeedForward(d)


class _Encoder(nn.Module):
    def __init__(self, blocks):
        super().__init__()
        self.blocks = nn.ModuleList(blocks)


class Mamba4RecModel(nn.Module):
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
    The model steps through calculate_loss / backward / torch.optim.Adam (``torch_optim``), on a single GPU."""

    needs_negatives = False
    needs_same_target = False
    torch_optim = True
    own_train_step = False
    full_logits = None                           # no dense-logits path: the rankings take last_hidden + catalogue_weight
    kernel_family = "Mamba"

    def __init__(self, args):
        super().__init__()
        if getattr(args, "storage", None) == "bf16" or (getattr(args, "plan_options", None) or {}).get("storage", 0):
            raise ValueError("Mamba4Rec: storage = 'bf16' does not apply (the Mamba kernels are fp32)")
        if getattr(args, "train_negatives", 0):
            raise ValueError("Mamba4Rec: train_negatives does not apply (the model has the full-catalogue cross-entropy)")
        if getattr(args, "train_lazy_adam", False):
            raise ValueError("Mamba4Rec: train_lazy_adam does not apply (the model steps through torch.optim.Adam)")
        self.args = args
        d, N = int(args.hidden_size), int(args.num_hidden_layers)
        if N < 1:
            raise ValueError(f"Mamba4Rec: num_hidden_layers = {N}, expected N >= 1")
        hyper = (int(getattr(args, "mamba_d_state", 16)), int(getattr(args, "mamba_d_conv", 4)),
                 int(getattr(args, "mamba_expand", 2)), getattr(args, "mamba_dt_rank", None))
        self.p_hidden = float(args.hidden_dropout_prob)
        if not 0.0 <= self.p_hidden < 1.0:
            raise ValueError(f"dropout probabilities must be in [0, 1), got {self.p_hidden}")
        self._actf = _act("gelu")
        std = float(args.initializer_range)
        self.item_embeddings = nn.Embedding(int(args.item_size), d)
        self.LayerNorm = _LayerNorm(d)
        self.item_encoder = _Encoder(_Block(d, *hyper, std) for _ in range(N))
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, (nn.Linear, nn.Embedding)):
                    m.weight.normal_(0.0, std)
                if isinstance(m, nn.Linear):
                    m.bias.zero_()
        self._ce_pool = {}                       # (B, V, d, device) -> free workspaces of bsarec_ce_head_*
        self._seed, self._rank, self._gen = 42, 0, None

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)         # every MambaLayer has flattened itself again by now
        self._gen, self._ce_pool = None, {}
        return out

    def check_trainer(self, args, process_group):
        """Called by Trainer before the first step."""
        if process_group is not None:
            raise ValueError("Mamba4Rec: single GPU only")

    def set_seed(self, seed: int, rank: int = 0):
        """Seed of the dropout draws (rank-decorrelated) of the torch generator."""
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
            raise ValueError(f"Mamba4Rec: input_ids must be [B, L], got {tuple(input_ids.shape)}")

    def _encode(self, input_ids, train: bool):
        """Every layer's output, [x0, x1, .. xN]."""
        ids = input_ids.to(torch.int64).contiguous()
        x = self._drop(self.LayerNorm(self.item_embeddings(ids)), train)
        outs = [x]
        for blk in self.item_encoder.blocks:
            ff = blk.feed_forward
            a = blk.mamba.LayerNorm(self._drop(blk.mamba(x, ids), train) + x)
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

    def grad_step(self, input_ids, answers, neg_answers=None):
        raise RuntimeError("Mamba4Rec steps through calculate_loss / backward / torch.optim.Adam (Trainer does)")
