"""FEARec sibling model: SASRec's encoder with the attention of every block replaced by a band-limited autocorrelation attention
(plus, optionally, a share of the causal softmax attention), trained with DuoRec's loss and a frequency-domain regulariser.

The contract of this model is the math of its docstrings, checked against an fp64 restatement (tests/fearec_ref.py,
tests/test_fearec_cpu.py); it was written from the FEARec paper without the reference source at hand, the defaults are the
reference's as remembered, and no reference golden exists for it yet.  The autocorrelation attention runs in libbsarec_hip.so in
both directions (bsarec_fea_attn_fwd / bsarec_fea_attn_bwd, csrc/fea_attn.h); the Linears, the LayerNorms, the softmax branch
and the loss are torch ops, the InfoNCE and catalogue-CE heads being DuoRec's (``duorec_head`` / ``duorec_ce_head``).  There is
no CPU path.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from . import _lib as L
from ._sibling import _Encoder, _FeedForward, _KernelLayer, _LayerNorm, _SiblingModel, _act, _no_cpu
from .model import duorec_head_options, duorec_loss

FREDOM_TYPES = ("un", "su", "us_x")
HIDDEN_ACTS = ("gelu", "relu", "swish", "tanh", "sigmoid")


def fea_bands(seq_len: int, num_layers: int, global_ratio: float):
    """[(lo, hi)] per layer: the rfft bins lo <= f < hi of F = L // 2 + 1 that the layer's cross-spectrum keeps.  Every band
    is ``w F`` bins wide and layer i sits ``i s`` bins below the top: N > 1 and ratio > 1 / N: w = ratio,
    s = (F (1 - ratio)) // (N - 1); N > 1 and ratio <= 1 / N: w = 1 / N, s = F / N; N = 1: w = max(ratio, 1), s = 0."""
    F, N, g = seq_len // 2 + 1, int(num_layers), float(global_ratio)
    if N < 1 or not 0.0 < g <= 1.0:
        raise ValueError(f"FEARec: num_hidden_layers = {N}, global_ratio = {g}: expected N >= 1 and a ratio in (0, 1]")
    if N > 1 and g > 1.0 / N:
        w, s = g, (F * (1 - g)) // (N - 1)
    elif N > 1:
        w, s = 1.0 / N, F / N
    else:
        w, s = max(g, 1.0 / N), 0
    out = []
    for i in range(N):
        lo, hi = int(F * (1 - w) - i * s), int(F - i * s)
        if not 0 <= lo < hi <= F:
            raise ValueError(f"FEARec: layer {i} of {N} has the empty or out-of-range band [{lo}, {hi}) of {F} bins "
                             f"(max_seq_length = {seq_len}, global_ratio = {g})")
        out.append((lo, hi))
    return out


def fea_topk(seq_len: int, factor: float = 1.0) -> int:
    """k = int(factor ln L), clamped to 1 .. min(L, 32)."""
    return max(1, min(int(float(factor) * math.log(seq_len)), seq_len, 32))


class FeaAttention(_KernelLayer):
    """q, k, v [B, L, D] -> out [B, L, D] on the HIP kernels, with F = L // 2 + 1 and the band lo <= f < hi:
      Qf[b, c, f] = sum_t q[b, t, c] e^{-2 pi i f t / L}  (Kf alike),   S[b, f] = sum_c Qf[b, c, f] conj(Kf[b, c, f])
      m[b, tau]   = 1 / (D L) sum_{f in band} w_f Re(S[b, f] e^{+2 pi i f tau / L});  w_f = 1 at f = 0 and at the Nyquist bin of
                    an even L, else 2 -- ``irfft(n = L)`` of the band-masked cross-spectrum, averaged over the channels
      idx         = the ``topk`` delays with the largest mean_b m[b, tau], shared by the batch (training mode), or with the
                    largest m[b, .] per sequence (evaluation mode); equal values go to the lower delay
      p[b, i]     = softmax_i(m[b, idx_i]),   out[b, t, c] = sum_i p[b, i] v[b, (t + idx_i) mod L, c]
    The head split plays no part (the correlation is averaged over heads and channels), and padding is not masked.  The
    backward is the true derivative with idx held fixed; nothing flows through the batch mean that only selects.  No
    parameters.  ``forward(q, k, v, train=None)``: the mode follows ``self.training`` unless ``train`` says otherwise.  The
    workspace carries m, the chosen delays and their softmax to the backward."""

    _tag, _kept = "fea_attn", "delays"

    def __init__(self, seq_len: int, width: int, lo: int, hi: int, topk: int):
        super().__init__()
        if not 2 <= seq_len <= 256:
            raise ValueError(f"FEARec: max_seq_length {seq_len} outside 2..256")
        if not (4 <= width <= 256 and width % 4 == 0):
            raise ValueError(f"FEARec: hidden_size {width} outside 4..256 or not a multiple of 4")
        if not 0 <= lo < hi <= seq_len // 2 + 1:
            raise ValueError(f"FEARec: band [{lo}, {hi}) is empty or outside the {seq_len // 2 + 1} rfft bins")
        if not 1 <= topk <= min(seq_len, 32):
            raise ValueError(f"FEARec: topk {topk} outside 1..{min(seq_len, 32)}")
        self.seq_len, self.width, self.lo, self.hi, self.topk = int(seq_len), int(width), int(lo), int(hi), int(topk)

    def extra_repr(self):
        return f"seq_len={self.seq_len}, width={self.width}, band=[{self.lo}, {self.hi}), topk={self.topk}"

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        self._pool = {}
        return out

    def _config(self, inputs, mode, train):
        q, k, v = inputs
        shape = (q.shape[0], self.seq_len, self.width) if q.dim() == 3 else None
        if shape is None or tuple(q.shape) != shape or tuple(k.shape) != shape or tuple(v.shape) != shape:
            raise ValueError(f"fea_attn: q, k and v must be [B, {self.seq_len}, {self.width}], got {tuple(q.shape)}, "
                             f"{tuple(k.shape)}, {tuple(v.shape)}")
        if not (q.is_cuda and k.is_cuda and v.is_cuda):
            raise _no_cpu()
        cfg = L.FeaAttnConfig(q.shape[0], self.seq_len, self.width, self.lo, self.hi, self.topk, int(mode))
        nbytes = L.load().bsarec_fea_attn_workspace_bytes(cfg)
        if nbytes < 0:
            raise ValueError(f"fea_attn: unsupported batch B = {q.shape[0]} (1 <= B <= 65536)")
        return cfg, nbytes

    def _fwd(self, cfg, inputs, mode, train, out, ws, nbytes, stream):
        q, k, v = inputs
        L.check(L.load().bsarec_fea_attn_fwd(cfg, q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes,
                                             stream), "bsarec_fea_attn_fwd")

    def _bwd(self, cfg, inputs, mode, flat, g, ws, nbytes, grads, dw, stream):
        q, k, v = inputs
        dq, dk, dv = grads
        L.check(L.load().bsarec_fea_attn_bwd(cfg, q.data_ptr(), k.data_ptr(), v.data_ptr(), g.data_ptr(), ws.data_ptr(), nbytes,
                                             dq.data_ptr(), dk.data_ptr(), dv.data_ptr(), stream), "bsarec_fea_attn_bwd")

    def forward(self, q, k, v, train=None):
        """Differentiable with respect to q, k and v when autograd is recording; otherwise the forward call alone.  The mode
        (``train``: delays shared by the batch) is the kernel's own flag and says nothing about a backward to come."""
        return self._call((q, k, v), self.training if train is None else bool(train))


class _FeaLayer(nn.Module):
    """``item_encoder.blocks.{i}.layer``: query / key / value / dense / LayerNorm under SASRec's names."""

    def __init__(self, d: int, heads: int, attn: FeaAttention):
        super().__init__()
        self.query, self.key, self.value, self.dense = nn.Linear(d, d), nn.Linear(d, d), nn.Linear(d, d), nn.Linear(d, d)
        self.LayerNorm = _LayerNorm(d)
        self.heads = heads
        self.fea = attn


class _Block(nn.Module):
    def __init__(self, d: int, heads: int, attn: FeaAttention):
        super().__init__()
        self.layer = _FeaLayer(d, heads, attn)
        self.feed_forward = _FeedForward(d)


class FEARecModel(_SiblingModel):
    """``bsarec_amd.main.MODEL_REGISTRY['fearec']`` (``--model_type FEARec``).  The module tree, the 4 + 16 N state_dict keys,
    their shapes and the init are SASRec's (``item_embeddings``, ``position_embeddings``, ``LayerNorm``,
    ``item_encoder.blocks.{i}.layer.{query,key,value,dense,LayerNorm}``, ``item_encoder.blocks.{i}.feed_forward.{dense_1,dense_2,
    LayerNorm}``): a SASRecModel state_dict of the same args loads into it, and the reverse.

    forward: x = Dropout(LN(E[ids] + P)); per block i, with band_i of ``fea_bands(L, N, global_ratio)`` and
    k = ``fea_topk(L, fea_topk_factor)``:
      Q, K, V = Linear(x);  ctx_f = FeaAttention(band_i, k)(Q, K, V)
      spatial_ratio r > 0: ctx_s = SASRec's causal multi-head softmax attention on the same Q, K, V (additive mask in
        {0, -10000} over padding keys and the future, dropout ``attention_probs_dropout_prob`` on the probabilities);
        ctx = (1 - r) ctx_f + r ctx_s.  At r = 0 the softmax branch is skipped.
      h = LN(Dropout(dense(ctx)) + x);  y = LN(Dropout(dense_2(act(dense_1(h)))) + h)
    LayerNorm is TF style with eps 1e-12; the dropout draws come from a torch generator seeded by ``set_seed``.  The filter
    is sized by L: ``input_ids.shape[1]`` must equal ``args.max_seq_length``.

    Loss: DuoRec's (``duorec_loss``: the catalogue CE of the last position plus the ``ssl`` variant's InfoNCE terms, with
    ``tau``, ``sim``, ``lmd``, ``lmd_sem``, ``duorec_head`` and ``duorec_ce_head`` as there).  With ``ssl = 'us_x'`` and
    ``fredom`` on it adds 0.1 mean|R(seq) - R(aug)| when ``fredom_type`` is 'un' or 'us_x' and 0.1 mean|R(seq) - R(sem)| when
    it is 'su' or 'us_x': R is the ortho-normalised rfft along the sequence axis of the whole [B, L, d] output, |.| the complex
    modulus, the mean over all B F d entries.  R of the DIFFERENCE is taken with two real [F, L] matrices (it is linear)."""

    needs_negatives = False
    needs_same_target = True
    torch_optim = True
    full_logits = None                           # no dense-logits path: the rankings take last_hidden + catalogue_weight
    kernel_family = "FEARec"
    model_name = "FEARec"

    def __init__(self, args):
        super().__init__(args)
        self._refuse_plan_options(args, "DuoRec's loss")
        d, Lq, N = int(args.hidden_size), int(args.max_seq_length), int(args.num_hidden_layers)
        heads = int(args.num_attention_heads)
        if d % heads != 0:
            raise ValueError(f"FEARec: hidden_size {d} is not a multiple of num_attention_heads {heads}")
        self.global_ratio = float(getattr(args, "global_ratio", 0.6))
        self.spatial_ratio = float(getattr(args, "spatial_ratio", 0.1))
        if not 0.0 <= self.spatial_ratio <= 1.0:
            raise ValueError(f"FEARec: spatial_ratio = {self.spatial_ratio}, expected a value in [0, 1]")
        factor = float(getattr(args, "fea_topk_factor", 1.0))
        if not 0.0 < factor < float("inf"):
            raise ValueError(f"FEARec: fea_topk_factor = {factor}, expected a finite number > 0")
        self.fredom = bool(getattr(args, "fredom", True))
        self.fredom_type = getattr(args, "fredom_type", "us_x")
        if self.fredom_type not in FREDOM_TYPES:
            raise ValueError(f"fredom_type must be one of {FREDOM_TYPES}, got {self.fredom_type!r}")
        act = getattr(args, "hidden_act", "gelu")
        if act not in HIDDEN_ACTS:
            raise KeyError(act)
        self._actf = _act(act)
        self.p_hidden, self.p_attn = float(args.hidden_dropout_prob), float(args.attention_probs_dropout_prob)
        for p in (self.p_hidden, self.p_attn):
            if not 0.0 <= p < 1.0:
                raise ValueError(f"dropout probabilities must be in [0, 1), got {p}")
        self.seq_len, self.bands, self.topk = Lq, fea_bands(Lq, N, self.global_ratio), fea_topk(Lq, factor)
        self.item_embeddings = nn.Embedding(int(args.item_size), d)
        self.position_embeddings = nn.Embedding(Lq, d)
        self.LayerNorm = _LayerNorm(d)
        self.item_encoder = _Encoder(_Block(d, heads, FeaAttention(Lq, d, lo, hi, self.topk)) for lo, hi in self.bands)
        std = float(args.initializer_range)
        with torch.no_grad():
            for m in self.modules():
                if isinstance(m, (nn.Linear, nn.Embedding)):
                    m.weight.normal_(0.0, std)
                if isinstance(m, nn.Linear):
                    m.bias.zero_()
        duorec_head_options(self, args)
        self._dft = {}

    def _apply(self, fn, recurse=True):
        out = super()._apply(fn, recurse)
        self._dft, self._nce_pool = {}, {}
        return out

    def _check_ids(self, input_ids):
        if input_ids.dim() != 2 or input_ids.shape[1] != self.seq_len:
            raise ValueError(f"FEARec: input_ids must be [B, max_seq_length = {self.seq_len}] (the bands are sized by it), "
                             f"got {tuple(input_ids.shape)}")

    def _spatial(self, layer, q, k, v, mask, train):
        B, Lq, d = q.shape
        h = layer.heads
        dh = d // h
        qh, kh, vh = (t.view(B, Lq, h, dh).transpose(1, 2) for t in (q, k, v))
        s = torch.matmul(qh, kh.transpose(-1, -2)) / math.sqrt(dh) + mask
        a = self._drop(torch.softmax(s, dim=-1), self.p_attn, train)
        return torch.matmul(a, vh).transpose(1, 2).reshape(B, Lq, d)

    def _encode(self, input_ids, train: bool):
        """Every layer's output, [x0, y1, .. yN]."""
        ids = input_ids.to(torch.int64)
        Lq, r = self.seq_len, self.spatial_ratio
        pos = torch.arange(Lq, device=ids.device)
        x = self._drop(self.LayerNorm(self.item_embeddings(ids) + self.position_embeddings(pos)[None]), self.p_hidden, train)
        mask = None
        if r > 0.0:
            ok = (ids > 0)[:, None, None, :] & torch.tril(torch.ones((Lq, Lq), dtype=torch.bool, device=ids.device))[None, None]
            mask = (1.0 - ok.to(x.dtype)) * -10000.0
        outs = [x]
        for blk in self.item_encoder.blocks:
            la, ff = blk.layer, blk.feed_forward
            q, k, v = la.query(x), la.key(x), la.value(x)
            ctx = la.fea(q, k, v, train=train)
            if r > 0.0:
                ctx = (1.0 - r) * ctx + r * self._spatial(la, q, k, v, mask, train)
            h = la.LayerNorm(self._drop(la.dense(ctx), self.p_hidden, train) + x)
            y = self._drop(ff.dense_2(self._actf(ff.dense_1(h))), self.p_hidden, train)
            x = ff.LayerNorm(y + h)
            outs.append(x)
        return outs

    def _dft_pair(self, ref):
        """The ortho-normalised rfft along the sequence axis as two real [F, L] matrices (cos / -sin over sqrt(L)), built in
        fp64 from exactly reduced arguments."""
        key = (ref.device, ref.dtype)
        if key not in self._dft:
            Lq = self.seq_len
            f = torch.arange(Lq // 2 + 1, dtype=torch.int64)[:, None]
            t = torch.arange(Lq, dtype=torch.int64)[None, :]
            ang = (f * t % Lq).to(torch.float64) * (2.0 * math.pi / Lq)
            s = 1.0 / math.sqrt(Lq)
            self._dft[key] = ((torch.cos(ang) * s).to(device=ref.device, dtype=ref.dtype),
                              (-torch.sin(ang) * s).to(device=ref.device, dtype=ref.dtype))
        return self._dft[key]

    def spectral_distance(self, a, b):
        """mean |R(a) - R(b)| over the B F d entries, R the ortho-normalised rfft along dim 1 of [B, L, d]."""
        C, S = self._dft_pair(a)
        diff = a - b
        re, im = torch.matmul(C, diff), torch.matmul(S, diff)
        return torch.abs(torch.complex(re, im)).mean()

    def calculate_loss(self, input_ids, answers, neg_answers=None, same_target=None, user_ids=None):
        """DuoRec's loss on whole sequences plus the frequency-domain regulariser (the class docstring): a 0-d tensor."""
        self._require_gpu(input_ids)
        if same_target is None and self.ssl in ("us", "su", "us_x"):
            raise ValueError(f"FEARec's loss with ssl = {self.ssl!r} needs same_target")
        loss, views = duorec_loss(self, self.forward, input_ids, answers, same_target)
        if self.ssl == "us_x" and self.fredom:
            if self.fredom_type in ("un", "us_x"):
                loss = loss + 0.1 * self.spectral_distance(views["seq"], views["aug"])
            if self.fredom_type in ("su", "us_x"):
                loss = loss + 0.1 * self.spectral_distance(views["seq"], views["sem"])
        return loss
