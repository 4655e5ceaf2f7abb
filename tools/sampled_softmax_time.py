"""ms per training step of the full-catalogue CE head against the sampled-softmax head (train_negatives = N), and the
time of the head's loss launches alone.  One configuration per process, so that a caller can give each its own time limit:

    python tools/sampled_softmax_time.py --V 100003 --neg 1024      # --neg 0: full-catalogue CE
    python tools/sampled_softmax_time.py --V 100003 --neg 1024 --lazy   # lazy Adam for the item table (train_lazy_adam)

Prints one JSON line.  B = 256, d = 64, L = 50, 2 layers, 2 heads, dropout 0.5 (the bench shape); eager bsarec_train_step."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--V", type=int, required=True)
    ap.add_argument("--neg", type=int, default=0)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--lazy", action="store_true", help="lazy (sparse) Adam for the item table (needs --neg > 0)")
    a = ap.parse_args()
    from bsarec_amd import BSARecModel
    B, L = 256, 50
    args = argparse.Namespace(item_size=a.V, hidden_size=64, max_seq_length=L, batch_size=B, hidden_dropout_prob=0.5,
                              attention_probs_dropout_prob=0.5, num_hidden_layers=2, num_attention_heads=2, hidden_act="gelu",
                              initializer_range=0.02, c=3, alpha=0.9, seed=42, train_negatives=a.neg,
                              train_lazy_adam=a.lazy)
    m = BSARecModel(args).cuda()
    m.configure_adam()
    m.train()
    rng = np.random.default_rng(0)
    ids = torch.from_numpy(rng.integers(1, a.V, size=(B, L)).astype(np.int64)).cuda()
    ans = torch.from_numpy(rng.integers(1, a.V, size=B).astype(np.int64)).cuda()
    for _ in range(a.warmup):
        m.train_step(ids, ans)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(a.steps):
        m.train_step(ids, ans)
    t1.record()
    torch.cuda.synchronize()
    step_ms = t0.elapsed_time(t1) / a.steps
    # the head's forward launches alone (bsarec_loss on the last forward): logits + CE, or draws + logits + CE
    plan = m._plan(B)
    st = m._stream()
    t0.record()
    for _ in range(a.steps):
        rc = plan.lib.bsarec_loss(plan.handle, C.c_void_p(ans.data_ptr()), st)
        assert rc == 0, rc
    t1.record()
    torch.cuda.synchronize()
    loss_ms = t0.elapsed_time(t1) / a.steps
    print(json.dumps({"V": a.V, "neg": a.neg, "lazy": a.lazy, "ms_per_step": round(step_ms, 4), "head_loss_ms": round(loss_ms, 4),
                      "head_loss_share": round(loss_ms / step_ms, 3)}), flush=True)


if __name__ == "__main__":
    main()
