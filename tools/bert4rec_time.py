#!/usr/bin/env python3
"""BERT4Rec's cloze step at B = 256, L = 50, d = 64, V = 3417, 2 layers, 2 heads, mask_ratio 0.2 (slots 20, capacity 5120 rows):

    python tools/bert4rec_time.py [--reps 100] [--warmup 20] > profiles/bert4rec_time.txt

  mask   bsarec_cloze_mask against a torch restatement of the rule on the device (torch.rand draws, cumulative sums, one
         nonzero -- which synchronises) and against the host list loop of the published implementations (random.random per item
         over Python lists, then the upload)
  head   forward + backward of the cloze head (bsarec_cloze_head_fwd / _bwd, the autograd node of BERT4RecModel) against
         index_select + matmul + F.cross_entropy + autograd on the same rows, with the peak memory of one call; at full
         sequences and at 9-item sequences, where about a fifth of the capacity is live
  step   calculate_loss + backward + torch.optim.Adam of BERT4RecModel with each head

One JSON line per measurement.  The variants alternate within one process, call by call; each time is a hipEvent pair around
one call (the host's enqueue work included) followed by a synchronise; the line gives the median and the min..max spread."""
import argparse
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from bsarec_amd import BERT4RecModel
from bsarec_amd.bert4rec import _ClozeHeadFn

C1 = dict(item_size=3417, hidden_size=64, max_seq_length=50, num_hidden_layers=2, num_attention_heads=2, hidden_dropout_prob=0.5,
          attention_probs_dropout_prob=0.5, initializer_range=0.02, hidden_act="gelu", c=3, seed=1, batch_size=256, mask_ratio=0.2)


def alternate(fns, reps, warmup):
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    times = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            ev[0].record(); fn(); ev[1].record()
            torch.cuda.synchronize()
            times[k].append(ev[0].elapsed_time(ev[1]))
    return {k: sorted(v) for k, v in times.items()}


def report(out, times):
    for k, t in times.items():
        out[k + "_ms"] = round(t[len(t) // 2], 4)
        out[k + "_spread_ms"] = [round(t[0], 4), round(t[-1], 4)]
    print(json.dumps(out), flush=True)


def peak_above_inputs(fn, pools):
    for p in pools:
        p.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - before) / 1e6, 2)


def torch_mask(seq, ratio, slots, mask_token):
    """The rule of bsarec_cloze_mask with torch.rand draws, on the device."""
    B, L = seq.shape
    real = seq > 0
    drawn = real & (torch.rand(B, L, device=seq.device) < ratio)
    none = ~drawn.any(1) & real[:, -1]
    drawn[:, -1] |= none
    after = drawn.flip(1).cumsum(1).flip(1) - drawn.long()                # drawn positions behind this one
    loss_pos = drawn & (after < slots)
    masked = torch.where(drawn, torch.full_like(seq, mask_token), seq)
    rows = loss_pos.reshape(-1).nonzero().view(-1)                        # (synchronises: the count comes to the host)
    return masked, rows.to(torch.int32), seq.reshape(-1)[rows]


def host_mask(seq_lists, ratio, slots, mask_token, device):
    """The published implementations' loop over Python lists, once per batch, and the upload."""
    masked, rows, targets = [], [], []
    L = len(seq_lists[0])
    for b, s in enumerate(seq_lists):
        m, pos = list(s), []
        for t, item in enumerate(s):
            if item > 0 and random.random() < ratio:
                m[t] = mask_token
                pos.append(t)
        if not pos and s[-1] > 0:
            m[-1] = mask_token
            pos.append(L - 1)
        for t in pos[-slots:]:
            rows.append(b * L + t)
            targets.append(s[t])
        masked.append(m)
    return (torch.tensor(masked, device=device), torch.tensor(rows, dtype=torch.int32, device=device),
            torch.tensor(targets, device=device))


class TorchHeadModel(BERT4RecModel):
    """The same step with index_select + matmul + F.cross_entropy + autograd as the head (rows x V logits)."""

    def calculate_loss(self, input_ids, answers, neg_answers=None, same_target=None, user_ids=None):
        seq = self.cloze_sequence(input_ids, answers)
        self._state[1:2].add_(1)
        masked, rows, targets, count = self.cloze_mask(seq)
        out = self.forward(masked, _new_step=False)
        return torch_head(out.reshape(-1, out.shape[-1]), self.item_embeddings.weight, rows, targets, count, self.num_items)


def torch_head(h, table, rows, targets, count, V):
    live = rows >= 0
    logits = torch.matmul(h.index_select(0, rows.clamp(min=0).long()), table[:V].T)
    per_row = torch.nn.functional.cross_entropy(logits, targets, reduction="none")
    return (per_row * live).sum() / count.clamp(min=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    B, L, V, d = C1["batch_size"], C1["max_seq_length"], C1["item_size"], C1["hidden_size"]
    model = BERT4RecModel(argparse.Namespace(**C1)).cuda().train()
    model.set_seed(1)
    slots = model.mask_slots
    full = torch.from_numpy(rng.integers(1, V, (B, L))).cuda()
    short = torch.zeros_like(full)
    short[:, L - 9:] = full[:, L - 9:]
    # ---- the mask
    lists = full.cpu().tolist()
    fns = {"hip": lambda: model.cloze_mask(full), "torch": lambda: torch_mask(full, 0.2, slots, V),
           "host": lambda: host_mask(lists, 0.2, slots, V, full.device)}
    out = {"what": "cloze mask", "B": B, "L": L, "ratio": 0.2, "slots": slots, "reps": a.reps,
           "live_rows_hip_torch": [int(model.cloze_mask(full)[3].item()), int(torch_mask(full, 0.2, slots, V)[1].numel())]}
    report(out, alternate(fns, a.reps, a.warmup))
    # ---- the head, at full and at 9-item sequences
    for name, seq in (("full sequences", full), ("9-item sequences", short)):
        masked, rows, targets, count = model.cloze_mask(seq)
        gen = torch.Generator(device="cuda").manual_seed(5)
        h = torch.randn(B, L, d, device="cuda", generator=gen).requires_grad_(True)
        E = (torch.randn(V + 1, d, device="cuda", generator=gen) / d ** 0.5).requires_grad_(True)

        def hip_head():
            h.grad = E.grad = None
            loss = _ClozeHeadFn.apply(model, h, E, rows, targets, count)
            loss.backward()
            return loss

        def ref_head():
            h.grad = E.grad = None
            loss = torch_head(h.reshape(-1, d), E, rows, targets, count, V)
            loss.backward()
            return loss

        out = {"what": "cloze head forward + backward, " + name, "capacity": B * slots, "live_rows": int(count.item()), "V": V,
               "d": d, "reps": a.reps, "loss_torch_hip": [round(ref_head().item(), 6), round(hip_head().item(), 6)]}
        hip_head()
        dh, dE = h.grad.clone(), E.grad.clone()
        ref_head()
        out["dh_rel_l2_hip_vs_torch"] = float(f"{float((dh - h.grad).norm() / h.grad.norm()):.2e}")
        out["dE_rel_l2_hip_vs_torch"] = float(f"{float((dE - E.grad).norm() / E.grad.norm()):.2e}")
        del dh, dE
        h.grad = E.grad = None
        out["torch_peak_MB"] = peak_above_inputs(ref_head, [])
        h.grad = E.grad = None
        out["hip_peak_MB"] = peak_above_inputs(hip_head, [model._ce_pool])
        report(out, alternate({"torch": ref_head, "hip": hip_head}, a.reps, a.warmup))
    # ---- the whole step with each head
    ans = torch.from_numpy(rng.integers(1, V, (B,))).cuda()
    models = {"hip": model, "torch": TorchHeadModel(argparse.Namespace(**C1)).cuda().train()}
    models["torch"].load_state_dict(model.state_dict())
    opts = {k: torch.optim.Adam(m.parameters(), lr=1e-3) for k, m in models.items()}

    def step(k):
        def run():
            loss = models[k].calculate_loss(full, ans)
            opts[k].zero_grad()
            loss.backward()
            opts[k].step()
        return run

    out = {"what": "calculate_loss + backward + Adam, by head", "B": B, "L": L, "d": d, "V": V, "reps": a.reps}
    report(out, alternate({k: step(k) for k in models}, a.reps, a.warmup))


if __name__ == "__main__":
    main()
