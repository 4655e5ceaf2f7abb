"""BERT4Rec (Sun et al., CIKM 2019) as a sibling model on the block kernels: ``--model_type BERT4Rec``.

The encoder is SASRec's (a BSARec plan with alpha = 0) with the plan option ``bidirectional``: attention under the padding mask
alone.  Training is the cloze task, every piece of it on the device and on the stream:

    masking   bsarec_cloze_mask      a Philox draw per token (site BSAREC_CLOZE_SITE of the step's dropout stream), the masked
                                     ids, and the compacted list of the positions that carry a loss
    encoder   bsarec_forward         on the masked ids, the same step's dropout masks; differentiable through
                                     bsarec_backward_seq
    loss      bsarec_cloze_head_*    full-catalogue cross-entropy on the listed rows of the [B, L, d] output, mean over the live
                                     count on the device, gradient scattered back into [B, L, d] -- no rows x V logits

The item table has V + 1 rows: id V is the mask token, which is an input only -- the classes of the loss and every ranking
are the items [0, V) (``catalogue_weight``).  Prediction appends the mask token to the history and reads its position.
The state_dict has SASRec's 36 keys, ``item_embeddings.weight`` being [V + 1, d].
"""
import copy
import math

import torch

from . import _lib as L
from .model import SASRecModel, _SlotToken


class _ClozeSeqFn(torch.autograd.Function):
    """The encoder on already-masked ids as an autograd node (model._SeqFn without the step advance: the caller advanced the
    counter once, and the masking read that step)."""

    @staticmethod
    def forward(ctx, model, ids, *params):
        B = ids.shape[0]
        slot = 1
        while (B, slot) in model._slots_busy:
            slot += 1
        model._slots_busy.add((B, slot))
        ctx.token = _SlotToken(model, (B, slot))
        plan = model._run_forward(ids, train=model.training, new_step=False, slot=slot)
        ctx.model, ctx.plan = model, plan
        N, Lq, d = model.args.num_hidden_layers, model.args.max_seq_length, model.args.hidden_size
        return plan.view(L.BUF_LAYER_OUT, N, (B, Lq, d)).clone()

    @staticmethod
    def backward(ctx, gout):
        model, plan = ctx.model, ctx.plan
        g = gout.to(torch.float32).contiguous()
        L.check(plan.lib.bsarec_backward_seq(plan.handle, g.data_ptr(), model._stream()), "bsarec_backward_seq")
        grads = model._garena.clone()
        ctx.token.release()
        return (None, None) + model._grads_in_param_order(grads)


def _f32_operand(t):
    t = t.detach()
    if t.dtype != torch.float32 or not t.is_contiguous() or t.data_ptr() % 16 != 0:
        t = t.to(torch.float32).contiguous()
    return t


def _cloze_head_fwd(model, seq, table, rows, targets, count):
    """bsarec_cloze_head_fwd on the [B, L, d] output ``seq``: (0-d loss, the workspace holding the row statistics, its pool
    key, (h, E, call) for the backward)."""
    h, E = _f32_operand(seq), _f32_operand(table)
    B, Lq, d = h.shape
    T, R, V = B * Lq, rows.shape[0], model.num_items
    lib = L.load()
    nbytes = lib.bsarec_cloze_head_workspace_bytes(R, V, d)
    if nbytes < 0:
        raise ValueError(f"cloze head: unsupported shape R = {R}, V = {V}, d = {d}")
    key = ("cloze", R, V, d, h.device)
    pool = model._ce_pool.setdefault(key, [])
    ws = pool.pop() if pool else torch.empty(nbytes, dtype=torch.uint8, device=h.device)
    loss = torch.empty(1, dtype=torch.float32, device=h.device)
    stream = torch.cuda.current_stream(h.device).cuda_stream
    L.check(lib.bsarec_cloze_head_fwd(h.data_ptr(), d, T, E.data_ptr(), R, V, d, rows.data_ptr(), targets.data_ptr(),
                                      count.data_ptr(), loss.data_ptr(), None, ws.data_ptr(), nbytes, stream),
            "bsarec_cloze_head_fwd")
    return loss[0], ws, key, (h, E, (T, R, V, d, nbytes))


class _ClozeHeadFn(torch.autograd.Function):
    """The cloze loss as one autograd node over bsarec_cloze_head_fwd / _bwd (model._CatalogueCeFn with a row list and a live
    count on the device).  ``table`` is the whole [V + 1, d] item table: the classes are its first V rows, and the gradient
    that comes back has a zero row for the mask token."""

    @staticmethod
    def forward(ctx, model, seq, table, rows, targets, count):
        loss, ws, key, (h, E, call) = _cloze_head_fwd(model, seq, table, rows, targets, count)
        ctx.save_for_backward(h, E, rows, targets, count)
        ctx.model, ctx.key, ctx.ws, ctx.call = model, key, ws, call
        return loss

    @staticmethod
    def backward(ctx, gout):
        h, E, rows, targets, count = ctx.saved_tensors
        T, R, V, d, nbytes = ctx.call
        if ctx.ws is None:
            raise RuntimeError("cloze head: backward ran twice (the forward's statistics are gone)")
        g = gout.to(torch.float32).reshape(1).contiguous()
        dh = torch.empty(h.shape, dtype=torch.float32, device=h.device)
        dE = torch.empty(E.shape, dtype=torch.float32, device=h.device)
        dE[V:].zero_()                                              # the mask token is not a class
        stream = torch.cuda.current_stream(h.device).cuda_stream
        L.check(L.load().bsarec_cloze_head_bwd(h.data_ptr(), d, T, E.data_ptr(), R, V, d, rows.data_ptr(), targets.data_ptr(),
                                               count.data_ptr(), g.data_ptr(), ctx.ws.data_ptr(), nbytes, dh.data_ptr(),
                                               dE.data_ptr(), stream), "bsarec_cloze_head_bwd")
        ctx.model._ce_pool[ctx.key].append(ctx.ws)
        ctx.ws = None
        return None, dh, dE, None, None, None


class BERT4RecModel(SASRecModel):
    """``SIBLING_MODELS['bert4rec'](args=args)`` (bsarec_amd.main).  ``args.mask_ratio`` (default 0.2): the share of the real
    positions replaced by the mask token in a training step; ``args.bert_mask_slots`` (default min(L, 2 ceil(ratio L))): loss
    positions kept per sequence, the capacity of the head's row list being batch x slots."""

    needs_negatives = False
    torch_optim = True                           # an arena model with an autograd loss, as DuoRec: torch.optim.Adam steps
    full_logits = None                           # no dense-logits path: the rankings take last_hidden + catalogue_weight

    def __init__(self, args):
        if getattr(args, "storage", None) == "bf16" or (getattr(args, "plan_options", None) or {}).get("storage", 0):
            raise ValueError("BERT4Rec: storage = 'bf16' does not apply (the cloze head and its encoder plans are fp32)")
        if getattr(args, "train_negatives", 0):
            raise ValueError("BERT4Rec: train_negatives does not apply (the model has its own cloze head)")
        if getattr(args, "train_lazy_adam", False):
            raise ValueError("BERT4Rec: train_lazy_adam does not apply (the model steps through torch.optim.Adam)")
        ratio = float(getattr(args, "mask_ratio", 0.2))
        if not 0.0 < ratio <= 1.0:                                   # (NaN fails both comparisons)
            raise ValueError(f"BERT4Rec: mask_ratio = {ratio}, expected a value in (0, 1]")
        Lq = int(args.max_seq_length)
        slots = getattr(args, "bert_mask_slots", None)
        slots = min(Lq, 2 * math.ceil(ratio * Lq)) if slots is None else int(slots)
        if not 1 <= slots <= Lq:
            raise ValueError(f"BERT4Rec: bert_mask_slots = {slots}, expected 1..{Lq}")
        V = int(args.item_size)                                      # the classes; the caller's args keep item_size = V
        a = copy.copy(args)
        a.item_size = V + 1                                          # the table and the plans: one more row, the mask token
        super().__init__(a)
        self.options["storage"] = 0
        self.num_items, self.mask_token = V, V
        self.mask_ratio, self.mask_slots = ratio, slots

    def check_trainer(self, args, process_group):
        """Called by Trainer before the first step."""
        if process_group is not None:
            raise ValueError("BERT4Rec: single GPU only")

    def _plan(self, batch: int, parity: int = 0, slot: int = 0):
        plan = super()._plan(batch, parity, slot)
        if not getattr(plan, "_bidirectional", False):
            L.check(plan.lib.bsarec_plan_set_bidirectional(plan.handle, 1), "bsarec_plan_set_bidirectional")
            plan._bidirectional = True
        return plan

    # ---- the cloze step -------------------------------------------------------------------------------
    def cloze_sequence(self, input_ids, answers):
        """[input_ids[:, 1:], answers]: the whole known prefix in the window that prediction uses."""
        dev = self._arena.device
        ids = input_ids.to(device=dev, dtype=torch.int64)
        return torch.cat((ids[:, 1:], answers.to(device=dev, dtype=torch.int64).view(-1, 1)), dim=1).contiguous()

    def cloze_mask(self, seq):
        """bsarec_cloze_mask at the model's current step: (masked ids [B, L], rows int32[B slots], targets int64[B slots],
        count int32[1]), all on the device."""
        self._require_gpu()
        if int(self._state[0].item()) == 0:
            self.set_seed(self._seed)
        B, Lq = seq.shape
        dev, R = seq.device, B * self.mask_slots
        masked = torch.empty_like(seq)
        rows = torch.empty(R, dtype=torch.int32, device=dev)
        targets = torch.empty(R, dtype=torch.int64, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        L.check(L.load().bsarec_cloze_mask(seq.data_ptr(), B, Lq, self.mask_ratio, self.mask_slots, self.mask_token,
                                           self._state.data_ptr(), masked.data_ptr(), rows.data_ptr(), targets.data_ptr(),
                                           count.data_ptr(), self._stream()), "bsarec_cloze_mask")
        return masked, rows, targets, count

    def calculate_loss(self, input_ids, answers, neg_answers=None, same_target=None, user_ids=None):
        """The cloze loss of one step: a 0-d tensor; ``.backward()`` fills every parameter's grad.  The step counter advances
        once (train mode); the masking and the encoder's dropout read that step.  In eval mode: the current step's masking,
        no dropout."""
        self._require_gpu()
        seq = self.cloze_sequence(input_ids, answers)
        if self.training:
            self._state[1:2].add_(1)
            self._step_begun = True
        masked, rows, targets, count = self.cloze_mask(seq)
        out = self.forward(masked, _new_step=False)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return _ClozeHeadFn.apply(self, out, self.item_embeddings.weight, rows, targets, count)
        loss, ws, key, _ = _cloze_head_fwd(self, out, self.item_embeddings.weight.detach(), rows, targets, count)
        self._ce_pool[key].append(ws)                                # no backward will read the statistics
        return loss

    # ---- reference model API ---------------------------------------------------------------------------
    def forward(self, input_ids, user_ids=None, all_sequence_output=False, _new_step=True):
        """The bidirectional encoder's [B, L, d].  ``_new_step = False``: the caller advanced the step counter itself."""
        if all_sequence_output or _new_step:
            return super().forward(input_ids, user_ids, all_sequence_output)
        if self.training and torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            return _ClozeSeqFn.apply(self, input_ids, *self.parameters())
        B, Lq, d = input_ids.shape[0], self.args.max_seq_length, self.args.hidden_size
        plan = self._run_forward(input_ids, train=self.training, new_step=False)
        return plan.view(L.BUF_LAYER_OUT, self.args.num_hidden_layers, (B, Lq, d)).clone()

    def _shift_in_mask(self, input_ids):
        ids = input_ids.to(device=self._arena.device, dtype=torch.int64)
        tail = torch.full((ids.shape[0], 1), self.mask_token, dtype=torch.int64, device=ids.device)
        return torch.cat((ids[:, 1:], tail), dim=1).contiguous()

    def last_hidden(self, input_ids) -> torch.Tensor:
        """The hidden state at the mask token appended to the history, [B, d] (a view into the plan's workspace)."""
        return super().last_hidden(self._shift_in_mask(input_ids))

    def predict(self, input_ids, user_ids=None, all_sequence_output=False):
        return self.last_hidden(input_ids).clone()

    def catalogue_weight(self) -> torch.Tensor:
        """The items a ranking scores: rows [0, V) of the table (the mask token is no item), detached."""
        return self.item_embeddings.weight.detach()[:self.num_items]

    def train_step(self, input_ids, answers, neg_answers=None):
        raise RuntimeError("BERT4Rec steps through calculate_loss / backward / torch.optim.Adam (Trainer does)")

    def grad_step(self, input_ids, answers, neg_answers=None):
        raise RuntimeError("BERT4Rec steps through calculate_loss / backward / torch.optim.Adam (Trainer does)")
