"""Catalogue-sharded BSARec training step (the C5 variant; include/bsarec_shard.h).

New functionality -- the reference is single-device (src/main.py:19).  At V = 10 M items and d = 256 a replicated item
table costs 41 GB per GPU (weights, gradient, Adam moments) and a dense 10.24 GB gradient all-reduce per step; here rank
r OWNS rows [r*rows_per, (r+1)*rows_per) of ``item_embeddings.weight`` -- their gradient and their Adam moments never
leave the GPU -- and the encoder (everything else, ~1.6 M parameters) stays a data-parallel replica.

What the reference does in `calculate_loss` (src/model/bsarec.py:30-37) maps to one step like this (per rank, B local
sequences, Bg = W*B):

  lookup           token rows are READ out of the owners' shards over xGMI (IPC-mapped hipMalloc memory) into a staging
                   table [B*L + 1, d]; the ordinary encoder plan runs over it with item_size = B*L + 1
  all-gather       h_last [Bg, d], answers [Bg], token ids [W, B*L]
  head             partial logits of ALL Bg sequences against the owned rows; per-row (max, sum exp, target logit)
  all-gather       the statistics [W, 3, Bg] -> lse, loss (identical on every rank), d loss / d logits of the owned slice
  head backward    dE of the owned rows: complete and local; partial d h_last -> all-reduce [Bg, d], keep the own rows
  encoder backward bsarec_backward_seq; the staging table's gradient holds one row per token
  barrier          (bsarec_comm_barrier) every rank's gradients are complete
  lookup gradient  owners PULL the token rows of their items out of every rank's staging gradient
  Adam             encoder: the fused Adam sums every rank's gradient arena in rank order (replicas stay bit-identical);
                   shard: local dE, local moments

The loss is the mean over the global batch: d loss / d logits carries 1 / Bg, so every gradient is already the
global-batch one and the encoder's Adam takes the plain SUM over ranks (grad_scale = 1).

Sampled-softmax head (opt-in, ``train_negatives`` N > 0 with ``train_sampler`` / ``train_no_logq`` / ``train_lazy_adam`` as on
one GPU) -- the head rows above become, per rank:

  draw             the step's N candidates, the same on every rank (key of set_seed(seed, rank=0), step = the encoder's
                   state[1] read on the device): those of ONE BSARecModel training on the global batch
  gather           the B answer rows and the N candidate rows out of the owners' shards
  head             logits / loss rows / d loss / d logits (1 / Bg) of the B local rows only; all-gather of the loss rows
  head backward    d h_last of the local rows (complete: no exchange); the head gradient rows [B + N, d] (IPC-exported)
  encoder backward, barrier   as above
  owner pull       every owner adds the answer rows of its items and the rank-ordered sum of the candidate partials
  Adam             shard: dense (dE zeroed once per step), or lazy over the owned rows the step touched

Full-catalogue CE without the partial logits (opt-in, ``shard_ce_head = "fused"``) -- the same loss and gradients as
the head rows of the first table, with no [Bg, Vs] buffer: between the all-gathers and the all-reduce of d h_last,

  statistics       ``bsarec_ce_head_range_stats`` over the owned rows with their column base: per-row (max, sum exp, target score)
  all-gather       the statistics [W, 3, Bg], as above
  merge            ``bsarec_ce_head_range_merge``: the whole catalogue's (max, log sum) per row, loss rows, loss (the same bits on
                   every rank)
  head backward    ``bsarec_ce_head_range_bwd``: the scores are formed again; dE of the owned rows and the partial d h_last

Evaluation (``topk`` / ``full_sort_scores``) ranks the owned rows for all Bg sequences and merges the ranks' lists.
``eval_full_rank`` (the single-GPU flag) picks how a rank gets its list: "dense" (default) materialises the partial logits
[Bg, Vs]; "fused" calls ``bsarec_topk_full_range`` over the shard with its column base -- O(Bg (s + cap)) working memory, no
score matrix, and under the sampled-softmax head no O(Bg Vs) buffer for the life of the object.  "rank" (``full_sort_scores``
only: it produces no lists) exchanges no candidates at all: the answers' scores (``bsarec_answer_score_range``) and the counts of
the owned items that stand before them (``bsarec_answer_rank_range``) are each summed over the ranks, 4 Bg bytes apiece.
"""
from __future__ import annotations

import copy
import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .dp import PeerExchange, _as_tensor
from .model import BSARecModel, train_head_of
from .ranking import (EVAL_FULL_RANK, REFERENCE_KS, FullRank, answer_rank, answer_score, cutoff_metrics, eval_full_rank_of,
                      metrics_post_fix, topk_seen)


SHARD_CE_HEADS = ("dense", "fused")


class ShardedCatalogue:
    """One rank of the catalogue-sharded step.  ``args`` are the reference's (global ``item_size``); ``batch`` is the
    per-rank batch size (fixed: the staging table and the encoder plan are sized by it)."""

    def __init__(self, args, batch: int, group, device):
        # the training head: full-catalogue CE, or the sampled-softmax head with the single-GPU flags and limits
        head = train_head_of(args)
        self.N = head["train_negatives"]
        self.popularity = head["train_sampler"] == L.TRAIN_SAMPLERS["popularity"]
        self.logq = 0 if head["train_no_logq"] else 1
        self.lazy = bool(getattr(args, "train_lazy_adam", False))
        if self.lazy and self.N == 0:
            raise ValueError("train_lazy_adam needs the sampled-softmax head (train_negatives > 0)")
        if getattr(args, "storage", None) == "bf16":
            raise ValueError("catalogue sharding is fp32 only")
        eval_full_rank_of(args)
        self.ce_head = getattr(args, "shard_ce_head", "dense")
        if self.ce_head not in SHARD_CE_HEADS:
            raise ValueError(f"shard_ce_head = {self.ce_head!r}, expected one of {SHARD_CE_HEADS}")
        if self.ce_head == "fused" and self.N:
            raise ValueError("shard_ce_head = 'fused' is the full-catalogue CE head: the sampled-softmax head "
                             f"(train_negatives = {self.N}) has no full CE")
        if torch.device(device).type != "cuda":        # before the process group, the IPC mappings and any allocation
            head_name = (f"sampled-softmax head, train_negatives = {self.N}" if self.N else "full-catalogue CE head")
            raise ValueError(f"ShardedCatalogue: the catalogue-sharded step ({head_name}) runs on the GPU only, "
                             f"not on device {str(device)!r}")
        import torch.distributed as dist
        self.args, self.group, self.device, self.B = args, group, torch.device(device), int(batch)
        self.rank, self.W = dist.get_rank(group), dist.get_world_size(group)
        if self.W > 8:
            raise ValueError("catalogue sharding runs inside one xGMI node (<= 8 ranks)")
        V, d, Lq = int(args.item_size), int(args.hidden_size), int(args.max_seq_length)
        self.V, self.d, self.Lq = V, d, Lq
        self.rows_per = (V + self.W - 1) // self.W
        self.lo = self.rank * self.rows_per
        self.Vs = max(0, min(self.rows_per, V - self.lo))
        self.n = self.B * Lq
        self.Bg = self.W * self.B
        self.lib = L.load()
        self._full_rank = FullRank("topk: eval_full_rank = 'fused' does not support Bg={B} Vs={V} d={d} k={k}")
        # encoder replica over the staging table
        enc_args = copy.copy(args)
        enc_args.item_size = self.n + 1
        enc_args.plan_options = dict(getattr(args, "plan_options", None) or {})
        enc_args.train_negatives, enc_args.train_lazy_adam = 0, False      # the head runs here, not in the encoder's plan
        self.encoder = BSARecModel(enc_args).to(self.device)
        off, self.stage_n, _ = self.encoder._slices["item_embeddings.weight"]
        assert off == 0 and self.stage_n == (self.n + 1) * d
        dist.broadcast(self.encoder._arena, src=dist.get_global_rank(group, 0), group=group)       # identical replicas
        self.encoder.set_seed(int(getattr(args, "seed", 42)), self.rank)
        # peer-to-peer plumbing: gradient arenas + the table shards in IPC-exported memory
        px = PeerExchange.create(self.encoder._numel, group, self.device)
        if px is None:
            raise RuntimeError("catalogue sharding needs the peer-to-peer mappings (hipIpc) between the ranks of the node")
        self.px = px
        self.encoder.use_grad_arenas(px.arenas)
        e_ptr, self.shard_ptrs = px.share(max(self.rows_per, 1) * d * 4)
        self.E = _as_tensor(e_ptr, self.rows_per * d, torch.float32, self.device).view(self.rows_per, d)
        gen = torch.Generator(device="cpu").manual_seed(int(getattr(args, "seed", 42)) * 1000003 + self.rank)
        self.E.copy_(torch.empty(self.rows_per, d).normal_(0.0, float(args.initializer_range), generator=gen))
        self.dE = torch.zeros_like(self.E)
        self.m, self.v = torch.zeros_like(self.E), torch.zeros_like(self.E)
        self.encoder.configure_adam(lr=float(getattr(args, "lr", 1e-3)),
                                    betas=(float(getattr(args, "adam_beta1", 0.9)), float(getattr(args, "adam_beta2", 0.999))),
                                    weight_decay=float(getattr(args, "weight_decay", 0.0)))
        # head buffers
        self.ld = (max(self.Vs, 1) + 3) // 4 * 4
        self.logits = self.h_all = None
        if self.N == 0:
            self.stats = torch.zeros(3, self.Bg, dtype=torch.float32, device=self.device)
            self.stats_all = torch.zeros(self.W, 3, self.Bg, dtype=torch.float32, device=self.device)
            self.dh = torch.zeros(self.Bg, d, dtype=torch.float32, device=self.device)
        if self.N == 0 and self.ce_head == "fused":     # no partial logits, no split-K scratch: the workspace of ce_head.h
            self._gathered_h_buffer()
            self.ce_ws_bytes = self.lib.bsarec_ce_head_range_workspace_bytes(self.Bg, self.Vs, d)
            if self.ce_ws_bytes <= 0:
                raise ValueError(f"shard_ce_head = 'fused' does not support Bg={self.Bg} Vs={self.Vs} d={d}")
            self.ce_ws = torch.zeros(self.ce_ws_bytes, dtype=torch.uint8, device=self.device)
            self.ce_g = torch.ones(1, dtype=torch.float32, device=self.device)
            self.ce_base = min(self.lo, V)          # a rank behind the last row owns the empty range [V, V)
        elif self.N == 0:
            self._full_head_buffers()
            self.scratch = torch.zeros(max(1, self.lib.bsarec_shard_head_bwd_scratch_floats(self.Bg, self.Vs, d)),
                                       dtype=torch.float32, device=self.device)
        self.ans_all = torch.zeros(self.Bg, dtype=torch.int64, device=self.device)
        self.ids_all = torch.zeros(self.W, self.n, dtype=torch.int64, device=self.device)
        self.local_ids = torch.zeros(self.B, Lq, dtype=torch.int64, device=self.device)
        self.d_out = torch.zeros(self.B, Lq, d, dtype=torch.float32, device=self.device)
        if self.N:
            self._sampled_head_buffers(px)
        self.loss_rows = torch.zeros(self.Bg, dtype=torch.float32, device=self.device)
        self.loss = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._shards8 = L.PTRS8(*([int(p) for p in self.shard_ptrs] + [None] * (8 - self.W)))
        self._grads8 = L.PTRS8(*([int(p) for p in px.grad_srcs(0)] + [None] * (8 - self.W)))
        dist.barrier(group=group)

    def _gathered_h_buffer(self):
        """The gathered h_last of all Bg sequences (the full-CE step; evaluation)."""
        if self.h_all is None:
            self.h_all = torch.zeros(self.Bg, self.d, dtype=torch.float32, device=self.device)

    def _full_head_buffers(self):
        """Partial logits of all Bg sequences against the owned rows, and the gathered h_last (the full-CE step; the dense
        evaluation)."""
        self._gathered_h_buffer()
        if self.logits is None:
            self.logits = torch.zeros(self.Bg, self.ld, dtype=torch.float32, device=self.device)

    def _sampled_head_buffers(self, px):
        B, N, d, dev = self.B, self.N, self.d, self.device
        # the draws' key: the one BSARecModel.set_seed(seed, rank=0) writes (the encoder replica's key is rank-decorrelated)
        self.key = int(getattr(self.args, "seed", 42)) & 0x7FFFFFFFFFFFFFFF
        self._cum = None                                            # set_train_popularity: device int64[V]
        self.cand = torch.zeros(N, dtype=torch.int32, device=dev)   # the step's candidates (tests read them)
        self.corr = torch.zeros(N, dtype=torch.float32, device=dev)
        self.rows = torch.zeros(B + N, d, dtype=torch.float32, device=dev)
        self.s_logits = torch.zeros(B, N + 1, dtype=torch.float32, device=dev)
        self.s_dlogits = torch.zeros(B, N + 1, dtype=torch.float32, device=dev)
        self.loss_rows_local = torch.zeros(B, dtype=torch.float32, device=dev)
        self.s_scratch = torch.zeros(self.lib.bsarec_shard_ssm_bwd_scratch_floats(B, N, d), dtype=torch.float32, device=dev)
        # the head gradient rows [B + N, d], read by the owners after the barrier that follows the backward
        g_ptr, g_ptrs = px.share((B + N) * d * 4)
        self.head_grad = _as_tensor(g_ptr, (B + N) * d, torch.float32, dev).view(B + N, d)
        self._hgrads8 = L.PTRS8(*([int(p) for p in g_ptrs] + [None] * (8 - self.W)))
        if self.lazy:       # the touched owned rows of a step (lazy_adam.h): marks [Vs] (0 between steps) and their list
            self.lazy_cap = min(self.Vs, self.W * self.n + self.Bg + N)
            self.lazy_mark = torch.zeros(max(self.Vs, 1), dtype=torch.int32, device=dev)
            self.lazy_rows = torch.zeros(max(self.lazy_cap, 1), dtype=torch.int32, device=dev)
            self.lazy_count = torch.zeros(1, dtype=torch.int32, device=dev)

    def set_train_popularity(self, counts):
        """The popularity sampler of the sampled-softmax head: ``counts`` int64[item_size] of item occurrences over the
        GLOBAL catalogue, the same on every rank (checks and format of BSARecModel.set_train_popularity)."""
        V = self.V
        c = np.asarray(counts, dtype=np.int64)
        if c.shape != (V,) or (c < 0).any():
            raise ValueError(f"set_train_popularity: expected {V} counts >= 0")
        cum = np.cumsum(np.where(np.arange(V) == 0, 0, c))
        if cum[-1] < 1:
            raise ValueError("set_train_popularity: every count is 0")
        if self.N and self._cum is not None:
            self._cum.copy_(torch.as_tensor(cum, dtype=torch.int64))   # in place: a captured step keeps its pointer
        elif self.N:
            self._cum = torch.as_tensor(cum, dtype=torch.int64, device=self.device)

    # ---- weights ---------------------------------------------------------------------------------------------------
    def load_full_state_dict(self, sd):
        """Reference-keyed state dict with the FULL item table: this rank keeps its rows and the encoder parameters."""
        full = sd["item_embeddings.weight"].to(device=self.device, dtype=torch.float32)
        assert tuple(full.shape) == (self.V, self.d)
        self.E.zero_()
        if self.Vs:
            self.E[:self.Vs].copy_(full[self.lo:self.lo + self.Vs])
        own = self.encoder.state_dict()
        for k in own:
            if k != "item_embeddings.weight":
                own[k].copy_(sd[k].to(device=self.device, dtype=torch.float32))
        torch.cuda.synchronize(self.device)
        torch.distributed.barrier(group=self.group)

    def check_exchange(self):
        """The barrier kernel gives up after 5 s and sets a STICKY error word instead of hanging; a step that ran past a
        timed-out barrier read incomplete peer memory.  Call once per epoch / before a checkpoint (``full_state_dict``
        does): the flag is MAX-reduced so that every rank raises."""
        bad = torch.tensor([1.0 if self.px.timed_out() else 0.0], device=self.device)
        torch.distributed.all_reduce(bad, op=torch.distributed.ReduceOp.MAX, group=self.group)
        if bad.item() != 0.0:
            raise RuntimeError("catalogue-sharded step: a cross-GPU barrier timed out on some rank (sticky error word); "
                               "shards and replicas can no longer be trusted")

    def full_state_dict(self):
        """The reference's state dict (full item table gathered from the owners; checkpoints of small catalogues, tests)."""
        self.check_exchange()
        parts = [torch.empty_like(self.E) for _ in range(self.W)]
        torch.distributed.all_gather(parts, self.E.contiguous(), group=self.group)
        sd = {k: v.detach().clone() for k, v in self.encoder.state_dict().items()}
        sd["item_embeddings.weight"] = torch.cat(parts, 0)[:self.V].clone()
        return sd

    # ---- one training step -----------------------------------------------------------------------------------------
    def _adam(self, params, grads, m, v, n, srcs=None):
        a = self.encoder._adam
        s = L.Adam(params, grads, m, v, n, a["lr"], a["b1"], a["b2"], a["eps"], a["wd"], 1.0, None, 0)
        if srcs:
            s.n_grad_srcs = len(srcs)
            for i, p in enumerate(srcs):
                s.grad_srcs[i] = p
        return s

    def train_step(self, input_ids, answers) -> torch.Tensor:
        """input_ids [B, L], answers [B]: this rank's slice of the global batch.  Returns the device loss scalar (mean
        over the GLOBAL batch, the same value on every rank)."""
        import torch.distributed as dist
        lib, enc, g = self.lib, self.encoder, self.group
        B, Lq, d, W, Bg, n = self.B, self.Lq, self.d, self.W, self.Bg, self.n
        ids = input_ids.to(device=self.device, dtype=torch.int64).contiguous()
        ans = answers.to(device=self.device, dtype=torch.int64).contiguous()
        assert tuple(ids.shape) == (B, Lq) and tuple(ans.shape) == (B,)
        if self.N and self.popularity and self._cum is None:
            raise ValueError("ShardedCatalogue: the popularity sampler needs set_train_popularity(counts) before the first step")
        st = enc._stream()
        # peers finished the previous step: their shards are current, nobody reads my old staging gradient any more
        self.px.barrier(st)
        L.check(lib.bsarec_shard_gather_rows(ids.data_ptr(), n, C.byref(self._shards8), W, self.rows_per, self.V, d,
                                             enc._arena.data_ptr(), self.local_ids.data_ptr(), st), "bsarec_shard_gather_rows")
        enc.train()
        plan = enc._run_forward(self.local_ids, train=True, new_step=True)
        if self.N:
            return self._sampled_step(plan, ids, ans, st)
        h_last = plan.view(L.BUF_LAYER_OUT, self.args.num_hidden_layers, (B, Lq, d))[:, Lq - 1, :].float().contiguous()
        dist.all_gather(list(self.h_all.view(W, B, d).unbind(0)), h_last, group=g)
        dist.all_gather(list(self.ans_all.view(W, B).unbind(0)), ans, group=g)
        dist.all_gather(list(self.ids_all.unbind(0)), ids.view(-1), group=g)
        if self.ce_head == "fused":
            self._fused_ce_head(st)
        else:
            self._dense_ce_head(st)
        dist.all_reduce(self.dh, op=dist.ReduceOp.SUM, group=g)
        self.d_out[:, Lq - 1, :] = self.dh[self.rank * B:(self.rank + 1) * B]
        L.check(lib.bsarec_backward_seq(plan.handle, self.d_out.data_ptr(), st), "bsarec_backward_seq")
        self.px.barrier(st)                 # every rank's gradient arena (staging rows + encoder) is complete
        L.check(lib.bsarec_shard_scatter_rows(self.ids_all.data_ptr(), n, W, C.byref(self._grads8), self.lo, self.Vs, self.V, d,
                                              self.dE.data_ptr(), st), "bsarec_shard_scatter_rows")
        sn, a = self.stage_n, enc._adam
        ad = self._adam(enc._arena.data_ptr() + 4 * sn, enc._garena.data_ptr() + 4 * sn, a["m"].data_ptr() + 4 * sn,
                        a["v"].data_ptr() + 4 * sn, enc._numel - sn, [p + 4 * sn for p in self.px.grad_srcs(0)])
        L.check(lib.bsarec_adam_step(C.byref(ad), enc._state.data_ptr(), st), "bsarec_adam_step")
        if self.Vs:
            ae = self._adam(self.E.data_ptr(), self.dE.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.Vs * d)
            L.check(lib.bsarec_adam_apply(C.byref(ae), enc._state.data_ptr(), st), "bsarec_adam_apply")
        return self.loss[0]

    def _dense_ce_head(self, st):
        """The full-CE head over the partial logits [Bg, Vs]: ``loss_rows``, ``loss``, ``dE`` of the owned rows and this rank's
        part of ``dh``, from ``h_all`` and ``ans_all``."""
        import torch.distributed as dist
        lib, d, W, Bg = self.lib, self.d, self.W, self.Bg
        L.check(lib.bsarec_shard_logits(self.h_all.data_ptr(), d, Bg, self.E.data_ptr(), self.Vs, d, self.logits.data_ptr(),
                                        self.ld, st), "bsarec_shard_logits")
        L.check(lib.bsarec_shard_ce_stats(self.logits.data_ptr(), self.ld, Bg, self.Vs, self.ans_all.data_ptr(), self.lo, self.V,
                                          self.stats.data_ptr(), st), "bsarec_shard_ce_stats")
        dist.all_gather(list(self.stats_all.unbind(0)), self.stats, group=self.group)
        L.check(lib.bsarec_shard_ce_grad(self.logits.data_ptr(), self.ld, Bg, self.Vs, self.ans_all.data_ptr(), self.lo, self.V,
                                         self.stats_all.data_ptr(), W, self.loss_rows.data_ptr(), self.loss.data_ptr(), st),
                "bsarec_shard_ce_grad")
        L.check(lib.bsarec_shard_head_bwd(self.logits.data_ptr(), self.ld, Bg, self.Vs, self.h_all.data_ptr(), d,
                                          self.E.data_ptr(), d, self.dE.data_ptr(), self.dh.data_ptr(), self.scratch.data_ptr(), st),
                "bsarec_shard_head_bwd")

    def _fused_ce_head(self, st):
        """The same outputs without the partial logits (``shard_ce_head = "fused"``): the range form of ce_head.h."""
        import torch.distributed as dist
        lib, d, W, Bg = self.lib, self.d, self.W, self.Bg
        h, E, a, ws = self.h_all.data_ptr(), self.E.data_ptr(), self.ans_all.data_ptr(), self.ce_ws.data_ptr()
        L.check(lib.bsarec_ce_head_range_stats(h, d, E, Bg, self.Vs, self.ce_base, self.V, d, a, self.stats.data_ptr(), ws,
                                               self.ce_ws_bytes, st), "bsarec_ce_head_range_stats")
        dist.all_gather(list(self.stats_all.unbind(0)), self.stats, group=self.group)
        L.check(lib.bsarec_ce_head_range_merge(self.stats_all.data_ptr(), W, Bg, ws, self.ce_ws_bytes, self.loss_rows.data_ptr(),
                                               self.loss.data_ptr(), st), "bsarec_ce_head_range_merge")
        L.check(lib.bsarec_ce_head_range_bwd(h, d, E, Bg, self.Vs, self.ce_base, self.V, d, a, self.ce_g.data_ptr(), ws,
                                             self.ce_ws_bytes, self.dh.data_ptr(), self.dE.data_ptr(), st),
                "bsarec_ce_head_range_bwd")

    def _sampled_step(self, plan, ids, ans, st) -> torch.Tensor:
        """The rest of :meth:`train_step` under the sampled-softmax head (module docstring; include/bsarec_shard.h)."""
        import torch.distributed as dist
        lib, enc, g = self.lib, self.encoder, self.group
        B, Lq, d, W, Bg, n, N = self.B, self.Lq, self.d, self.W, self.Bg, self.n, self.N
        H = plan.view(L.BUF_LAYER_OUT, self.args.num_hidden_layers, (B, Lq, d))
        h, ldh = H.data_ptr() + 4 * (Lq - 1) * d, Lq * d          # h_last in place: row b at position L-1
        cum = self._cum.data_ptr() if self.popularity else None
        dist.all_gather(list(self.ans_all.view(W, B).unbind(0)), ans, group=g)
        dist.all_gather(list(self.ids_all.unbind(0)), ids.view(-1), group=g)
        if not self.lazy:
            self.dE.zero_()                 # the head adds its rows now: no dense overwrite of the owned rows any more
        L.check(lib.bsarec_shard_ssm_draw(self.key, enc._state.data_ptr(), N, self.V, cum, self.logq, self.cand.data_ptr(),
                                          self.corr.data_ptr(), self.lazy_count.data_ptr() if self.lazy else None, st),
                "bsarec_shard_ssm_draw")
        L.check(lib.bsarec_shard_ssm_gather(ans.data_ptr(), B, self.cand.data_ptr(), N, C.byref(self._shards8), W, self.rows_per,
                                            self.V, d, self.rows.data_ptr(), st), "bsarec_shard_ssm_gather")
        L.check(lib.bsarec_shard_ssm_head(h, ldh, B, Bg, self.rows.data_ptr(), ans.data_ptr(), self.cand.data_ptr(),
                                          self.corr.data_ptr(), N, self.V, cum, self.logq, d, self.s_logits.data_ptr(),
                                          self.s_dlogits.data_ptr(), self.loss_rows_local.data_ptr(), st), "bsarec_shard_ssm_head")
        dist.all_gather(list(self.loss_rows.view(W, B).unbind(0)), self.loss_rows_local, group=g)
        L.check(lib.bsarec_shard_ssm_loss(self.loss_rows.data_ptr(), Bg, self.loss.data_ptr(), st), "bsarec_shard_ssm_loss")
        L.check(lib.bsarec_shard_ssm_bwd(self.s_dlogits.data_ptr(), B, N, h, ldh, self.rows.data_ptr(), d,
                                         self.d_out.data_ptr() + 4 * (Lq - 1) * d, Lq * d, self.head_grad.data_ptr(),
                                         self.s_scratch.data_ptr(), st), "bsarec_shard_ssm_bwd")
        L.check(lib.bsarec_backward_seq(plan.handle, self.d_out.data_ptr(), st), "bsarec_backward_seq")
        self.px.barrier(st)                 # every rank's gradient arena and head gradient rows are complete
        L.check(lib.bsarec_shard_ssm_pull(self.ans_all.data_ptr(), B, W, self.cand.data_ptr(), N, C.byref(self._hgrads8), self.lo,
                                          self.Vs, self.V, d, self.dE.data_ptr(), st), "bsarec_shard_ssm_pull")
        L.check(lib.bsarec_shard_scatter_rows(self.ids_all.data_ptr(), n, W, C.byref(self._grads8), self.lo, self.Vs, self.V, d,
                                              self.dE.data_ptr(), st), "bsarec_shard_scatter_rows")
        sn, a = self.stage_n, enc._adam
        ad = self._adam(enc._arena.data_ptr() + 4 * sn, enc._garena.data_ptr() + 4 * sn, a["m"].data_ptr() + 4 * sn,
                        a["v"].data_ptr() + 4 * sn, enc._numel - sn, [p + 4 * sn for p in self.px.grad_srcs(0)])
        L.check(lib.bsarec_adam_step(C.byref(ad), enc._state.data_ptr(), st), "bsarec_adam_step")
        if self.Vs and self.lazy:
            L.check(lib.bsarec_shard_lazy_mark(self.ids_all.data_ptr(), W * n, self.ans_all.data_ptr(), Bg, self.cand.data_ptr(), N,
                                               self.lo, self.Vs, self.V, self.lazy_mark.data_ptr(), self.lazy_rows.data_ptr(),
                                               self.lazy_count.data_ptr(), self.lazy_cap, st), "bsarec_shard_lazy_mark")
            L.check(lib.bsarec_shard_lazy_adam(self.E.data_ptr(), self.dE.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), d,
                                               a["b1"], a["b2"], a["eps"], a["wd"], self.lazy_mark.data_ptr(),
                                               self.lazy_rows.data_ptr(), self.lazy_count.data_ptr(), self.lazy_cap,
                                               enc._state.data_ptr(), st), "bsarec_shard_lazy_adam")
        elif self.Vs:
            ae = self._adam(self.E.data_ptr(), self.dE.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), self.Vs * d)
            L.check(lib.bsarec_adam_apply(C.byref(ae), enc._state.data_ptr(), st), "bsarec_adam_apply")
        return self.loss[0]

    def train_step_graph(self, input_ids, answers) -> torch.Tensor:
        """:meth:`train_step` replayed from ONE hipGraph: the kernels AND the collectives between them (all-gathers of
        h_last / answers / ids / statistics, the all-reduce of d h_last -- torch.distributed over RCCL enqueues them on the
        capture stream, as the data-parallel step's in-graph all-reduce does) are captured once for this rank's static
        input buffers; every later call copies the batch in and launches the graph: no host work between the step's ~25
        launches.  The first call runs eagerly (plans, kernel attributes, communicators) and captures; if the backend's
        collectives cannot be captured (gloo in the tests) the step stays eager -- ``graph_captured`` says which."""
        ids = input_ids.to(device=self.device, dtype=torch.int64).contiguous()
        ans = answers.to(device=self.device, dtype=torch.int64).contiguous()
        if getattr(self, "_graph", None) is None and not getattr(self, "_graph_failed", False):
            self._sid, self._sans = ids.clone(), ans.clone()
            loss = self.train_step(self._sid, self._sans).clone()
            torch.cuda.synchronize(self.device)
            try:
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    gl = self.train_step(self._sid, self._sans)
                self._graph = (g, gl)
            except Exception as e:                    # capture of a collective refused: eager from now on
                self._graph_failed, self._graph_error = True, f"{type(e).__name__}: {e}"
                torch.cuda.synchronize(self.device)
            return loss
        if getattr(self, "_graph", None) is not None:
            self._sid.copy_(ids)
            self._sans.copy_(ans)
            self._graph[0].replay()
            return self._graph[1]
        return self.train_step(ids, ans)

    @property
    def graph_captured(self) -> bool:
        return getattr(self, "_graph", None) is not None

    # ---- evaluation ------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def topk(self, input_ids, k: int = 20, seen=None, full_rank=None):
        """Full-catalogue top-k of this rank's B sequences over the SHARDED table (the reference's eval step,
        src/trainers.py:118-141: scores of the last position against every item, items the user already interacted
        with set to 0 -- not -inf --, top 20): local scores of all Bg sequences against the owned rows, local top-k,
        all-gather of the W x k candidates, merge.  ``seen``: optional int64 [B, S] of item ids per sequence (padded with
        -1).  ``full_rank``: "dense" (the partial logits [Bg, Vs], then ``bsarec_topk_seen``) or "fused"
        (``bsarec_topk_full_range`` over the owned rows: no score matrix); None: ``args.eval_full_rank``, else "dense".
        Returns (scores [B, k], item ids [B, k])."""
        import torch.distributed as dist
        mode = eval_full_rank_of(self.args, full_rank)
        if mode == "rank":                  # before any collective
            raise ValueError("topk: eval_full_rank = 'rank' produces no lists; use full_sort_scores(full_rank='rank')")
        fused = mode == "fused"
        lib, g, st = self.lib, self.group, self.encoder._stream()
        B, d, W, Bg = self.B, self.d, self.W, self.Bg
        seen_all = self._gather_h_and_seen(input_ids, seen, dense=not fused)
        if not fused:
            S = seen_all.shape[2] if seen_all is not None else 0
            L.check(lib.bsarec_shard_logits(self.h_all.data_ptr(), d, Bg, self.E.data_ptr(), self.Vs, d, self.logits.data_ptr(),
                                            self.ld, st), "bsarec_shard_logits")
            scores = self.logits[:, :self.Vs]
            if seen_all is not None:
                loc = seen_all.view(Bg, S) - self.lo
                ok = (seen_all.view(Bg, S) >= 0) & (loc >= 0) & (loc < self.Vs)
                rows = torch.arange(Bg, device=self.device).view(Bg, 1).expand(Bg, S)
                scores[rows[ok], loc[ok]] = 0.0
        if not 1 <= k <= min(L.TOPK_MAX, self.V):
            raise ValueError(f"topk: k = {k} outside 1 .. min(BSAREC_TOPK_MAX = {L.TOPK_MAX}, items = {self.V})")
        # rank r contributes its min(k, Vs_r) best; the gathered blocks are padded to k, and the merge reads only the real
        # candidates, in rank order: equal scores then stand in global id order (shards are contiguous id ranges and each
        # block is in ascending id order among its ties), so the merge's "smaller column first" is the full table's order
        n_r = [min(k, max(0, min(self.rows_per, self.V - r * self.rows_per))) for r in range(W)]
        kk = n_r[self.rank]
        cand_v = torch.zeros(Bg, k, device=self.device)
        cand_i = torch.zeros(Bg, k, dtype=torch.int64, device=self.device)
        if kk and fused:
            cand_v[:, :kk], cand_i[:, :kk] = self._topk_range(seen_all, kk)
        elif kk:
            i, v = topk_seen(scores, kk, values=True)
            cand_v[:, :kk], cand_i[:, :kk] = v, i + self.lo
        all_v = torch.empty(W, Bg, k, device=self.device)
        all_i = torch.empty(W, Bg, k, dtype=torch.int64, device=self.device)
        dist.all_gather(list(all_v.unbind(0)), cand_v, group=g)
        dist.all_gather(list(all_i.unbind(0)), cand_i, group=g)
        real = torch.cat([torch.arange(r * k, r * k + n, device=self.device) for r, n in enumerate(n_r) if n])
        mv = all_v.permute(1, 0, 2).reshape(Bg, W * k)[:, real].contiguous()
        mi = all_i.permute(1, 0, 2).reshape(Bg, W * k)[:, real]
        sel, top_v = topk_seen(mv, k, values=True)
        top_i = torch.gather(mi, 1, sel)
        r0 = self.rank * B
        return top_v[r0:r0 + B].clone(), top_i[r0:r0 + B].clone()

    def _gather_h_and_seen(self, input_ids, seen, dense: bool):
        """The evaluation forward of this rank's B sequences and the all-gathers every evaluation path starts with: h_last of
        all Bg sequences into ``h_all``; returns the gathered ``seen`` int64 [W, B, S], or None.  ``dense``: the caller needs
        the partial-logits buffer too."""
        import torch.distributed as dist
        lib, enc, g = self.lib, self.encoder, self.group
        B, Lq, d, W, n = self.B, self.Lq, self.d, self.W, self.n
        ids = input_ids.to(device=self.device, dtype=torch.int64).contiguous()
        assert tuple(ids.shape) == (B, Lq)
        st = enc._stream()
        if dense:                           # sampled-softmax training: the full-catalogue buffers on the first dense evaluation
            self._full_head_buffers()
        else:                               # the gathered h_last only
            self._gathered_h_buffer()
        self.px.barrier(st)
        L.check(lib.bsarec_shard_gather_rows(ids.data_ptr(), n, C.byref(self._shards8), W, self.rows_per, self.V, d,
                                             enc._arena.data_ptr(), self.local_ids.data_ptr(), st), "bsarec_shard_gather_rows")
        was_training = enc.training
        enc.eval()
        plan = enc._run_forward(self.local_ids, train=False, new_step=False)
        enc.train(was_training)
        h_last = plan.view(L.BUF_LAYER_OUT, self.args.num_hidden_layers, (B, Lq, d))[:, Lq - 1, :].float().contiguous()
        dist.all_gather(list(self.h_all.view(W, B, d).unbind(0)), h_last, group=g)
        if seen is None:
            return None
        sl = seen.to(device=self.device, dtype=torch.int64).contiguous()
        seen_all = torch.empty(W, B, sl.shape[1], dtype=torch.int64, device=self.device)
        dist.all_gather(list(seen_all.unbind(0)), sl, group=g)
        return seen_all

    def _seen_rows(self, seen_all):
        """``seen_all`` int64 [W, B, S] as (users, csr) of S entries per row; -1 pads and other ranks' items lie outside the range."""
        if seen_all is None:
            return None, None
        return (torch.arange(self.Bg, dtype=torch.int64, device=self.device),
                (torch.arange(self.Bg + 1, dtype=torch.int64, device=self.device) * seen_all.shape[2], seen_all))

    @torch.no_grad()
    def answer_ranks(self, input_ids, answers, seen=None):
        """The full-catalogue ranks (int32 [B], 0 = first; -1: an answer outside [0, V)) of this rank's B answers over the
        SHARDED table, in the order of :meth:`topk`, without lists: every rank scores the answers it owns into a zeroed [Bg]
        buffer (all-reduce SUM: x + 0 = x), counts the owned items that stand before each of the Bg answers, and the counts
        are all-reduced.  Two exchanges of 4 Bg bytes after the gathers of h_last, the answers and ``seen``."""
        import torch.distributed as dist
        g, B, W, Bg = self.group, self.B, self.W, self.Bg
        seen_all = self._gather_h_and_seen(input_ids, seen, dense=False)
        dist.all_gather(list(self.ans_all.view(W, B).unbind(0)), answers.to(device=self.device, dtype=torch.int64).contiguous(),
                        group=g)
        users, csr = self._seen_rows(seen_all)
        score = torch.zeros(Bg, dtype=torch.float32, device=self.device)
        rank = torch.zeros(Bg, dtype=torch.int32, device=self.device)
        if self.Vs:
            answer_score(self.h_all, self.E[:self.Vs], self.ans_all, users, csr, base=self.lo, out=score)
        dist.all_reduce(score, op=dist.ReduceOp.SUM, group=g)
        if self.Vs:
            rank = answer_rank(self.h_all, self.E[:self.Vs], self.ans_all, users, csr, base=self.lo, answer_score=score)
        dist.all_reduce(rank, op=dist.ReduceOp.SUM, group=g)
        rank[(self.ans_all < 0) | (self.ans_all >= self.V)] = -1      # (every owner said -1, or nobody owns the id)
        r0 = self.rank * B
        return rank[r0:r0 + B].clone()

    def _topk_range(self, seen_all, k):
        """k best owned items of all Bg rows of ``h_all`` (``FullRank`` over the shard, column base ``lo``): (scores, GLOBAL ids).
        ``seen_all`` int64 [W, B, S] or None: a CSR of S entries per row; -1 pads and other ranks' items lie outside the range."""
        users, csr = self._seen_rows(seen_all)
        idx, val = self._full_rank(self.h_all, self.E[:self.Vs], k, users, csr, base=self.lo, values=True)
        return val, idx

    @torch.no_grad()
    def full_sort_scores(self, batches, epoch: int = 0, k: int = 20, extra_ks=(), full_rank=None):
        """The reference's evaluation bookkeeping (src/trainers.py:118-158 + get_full_sort_score, :70-83) over the SHARDED
        table: ``batches`` yields this rank's (input_ids [B, L], answers [B], seen [B, S] or None) per step (every rank the
        same number of steps); the top-max(k, *extra_ks) of each sequence comes from :meth:`topk`, hits and DCG sums are
        all-reduced, so every rank returns the metrics of the GLOBAL evaluation set: ([HR@5, NDCG@5, HR@10, NDCG@10, HR@20,
        NDCG@20] + [HR@e, NDCG@e for e in extra_ks], str).  ``full_rank``: as in :meth:`topk`, or "rank": the same values from
        :meth:`answer_ranks` -- no lists, no candidate gathers, no merge, and cutoffs of any depth."""
        import torch.distributed as dist
        ks = REFERENCE_KS + tuple(extra_ks or ())
        depth = max((k,) + ks[3:])
        sums = torch.zeros(2 * len(ks) + 1, dtype=torch.float64, device=self.device)
        by_rank = eval_full_rank_of(self.args, full_rank) == "rank"
        for ids, answers, seen in batches:
            if by_rank:                     # no lists: the answers' ranks (an answer outside the catalogue never hits)
                r = self.answer_ranks(ids, answers, seen).cpu().numpy().astype(np.int64)
                n = r.shape[0]
                vals = cutoff_metrics(ks, ranks=np.where(r < 0, self.V, r))
            else:
                _, top_i = self.topk(ids, k=depth, seen=seen, full_rank=full_rank)
                hit = top_i == answers.to(device=self.device, dtype=torch.int64).view(-1, 1)
                n = hit.shape[0]
                vals = cutoff_metrics(ks, hit=hit)
            sums[:-1] += torch.tensor(vals, dtype=torch.float64, device=self.device) * n
            sums[-1] += n
        dist.all_reduce(sums, op=dist.ReduceOp.SUM, group=self.group)
        vals = (sums[:-1] / sums[-1].clamp(min=1)).tolist()
        return vals, str(metrics_post_fix(epoch, ks, vals))

    def close(self):
        torch.cuda.synchronize(self.device)
        torch.distributed.barrier(group=self.group)
        self.px.close()
