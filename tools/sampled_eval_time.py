#!/usr/bin/env python3
"""Time sampled-candidate evaluation against the full ranking, per batch of B = 256 sequences at hidden 64, with hipEvents
after warm-up.

    python tools/sampled_eval_time.py [--reps 20] [--items 3417,1000003] [--out FILE]

One JSON line per catalogue size V: milliseconds per batch of
  * sampled (N = 100, uniform and two popularity tables): model.last_hidden + bsarec_sampled_rank (ranks, candidates, scores);
  * full: model.full_logits + bsarec_topk_seen (k = 20, seen items masked) -- the default evaluation;
and of the two kernels alone (bsarec_sampled_rank on a fixed hidden state; bsarec_topk_seen on the logits of one forward,
restored before every call outside the timed region).  The seen rows are ML-1M-shaped (lognormal lengths, 20..2314 items,
uniform items); popularity counts are proportional to 1 / rank ("popularity") or Zipf(1.6) samples with 20 % zeros
("popularity_skewed").  A 2-layer, 2-head BSARec at max_seq_length 50."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from bsarec_amd import BSARecModel, _lib as Lb


def timed(fn, reps, reset=None):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps)]
    for _ in range(3):
        if reset:
            reset()
        fn()
    for r in range(reps):
        if reset:
            reset()
        ev[2 * r].record(); fn(); ev[2 * r + 1].record()
    torch.cuda.synchronize()
    return sum(ev[2 * r].elapsed_time(ev[2 * r + 1]) for r in range(reps)) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--items", default="3417,1000003")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--negatives", type=int, default=100)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lib = Lb.load()
    st = torch.cuda.current_stream().cuda_stream
    B, L, d, n = a.batch, 50, 64, a.negatives
    lines = []
    for V in (int(v) for v in a.items.split(",")):
        rng = np.random.default_rng(V)
        args = argparse.Namespace(item_size=V, hidden_size=d, max_seq_length=L, batch_size=B, hidden_dropout_prob=0.5,
                                  attention_probs_dropout_prob=0.5, num_hidden_layers=2, num_attention_heads=2, hidden_act="gelu",
                                  initializer_range=0.02, c=3, alpha=0.9, seed=1)
        torch.manual_seed(0)
        model = BSARecModel(args).cuda()
        model.eval()
        ids = torch.as_tensor(rng.integers(1, V, size=(B, L)), device="cuda")
        lens = np.clip(np.rint(rng.lognormal(4.6, 0.9, size=B)), 20, min(2314, V // 2)).astype(np.int64)
        rows = [np.unique(rng.integers(1, V, size=m)) for m in lens]
        indptr = torch.as_tensor(np.concatenate([[0], np.cumsum([len(r) for r in rows])]), device="cuda")
        indices = torch.as_tensor(np.concatenate(rows), device="cuda")
        users = torch.arange(B, device="cuda")
        ans_np = np.array([int(rng.choice(np.setdiff1d(np.arange(1, min(V, 2 * len(r) + 2)), r))) for r in rows])
        answers = torch.as_tensor(ans_np, device="cuda")
        # popularity: counts proportional to 1 / rank over a random permutation (the Zipf(1.0) of data.synth_ml1m_like);
        # popularity_skewed: Zipf(1.6) samples with 20 % zeros -- a few items hold most of the mass, so most draws repeat
        # an item already drawn and a row needs many rounds to reach N distinct negatives
        pop = np.zeros(V, dtype=np.int64)
        pop[1 + rng.permutation(V - 1)] = np.maximum(1, (10 ** 6 / np.arange(1, V)).astype(np.int64))
        skew = rng.zipf(1.6, size=V).astype(np.int64)
        skew[rng.random(V) < 0.2] = 0
        skew[0] = 0
        skew[ans_np] = np.maximum(skew[ans_np], 1)
        cums = {"popularity": torch.as_tensor(np.cumsum(pop), device="cuda"),
                "popularity_skewed": torch.as_tensor(np.cumsum(skew), device="cuda")}
        E = model.item_embeddings.weight.detach()
        rank = torch.empty(B, dtype=torch.int32, device="cuda")
        cand = torch.empty(B, n + 1, dtype=torch.int64, device="cuda")
        score = torch.empty(B, n + 1, device="cuda")
        idx = torch.empty(B, 20, dtype=torch.int64, device="cuda")

        def sampled_kernel(h, pc):
            Lb.check(lib.bsarec_sampled_rank(h.data_ptr(), h.stride(0), E.data_ptr(), B, V, d, users.data_ptr(), answers.data_ptr(),
                                             indptr.data_ptr(), indices.data_ptr(), pc, n, 7, 1, rank.data_ptr(), cand.data_ptr(),
                                             score.data_ptr(), st), "bsarec_sampled_rank")

        def topk_kernel(s):
            Lb.check(lib.bsarec_topk_seen(s.data_ptr(), s.stride(0), B, V, users.data_ptr(), indptr.data_ptr(), indices.data_ptr(), 20,
                                          idx.data_ptr(), None, st), "bsarec_topk_seen")

        out = {"B": B, "V": V, "d": d, "N": n, "k": 20}
        for name, pc in [("uniform", None)] + [(k, c.data_ptr()) for k, c in cums.items()]:
            out[f"sampled_{name}_ms"] = round(timed(lambda: sampled_kernel(model.last_hidden(ids), pc), a.reps), 4)
            h = model.last_hidden(ids).clone()
            out[f"sampled_{name}_kernel_ms"] = round(timed(lambda: sampled_kernel(h, pc), a.reps), 4)
            torch.cuda.synchronize()
            out[f"sampled_{name}_failed_rows"] = int((rank < 0).sum().item())
        out["full_ms"] = round(timed(lambda: topk_kernel(model.full_logits(ids)), a.reps), 4)
        logits = model.full_logits(ids).clone()
        work = logits.clone()
        out["full_topk_kernel_ms"] = round(timed(lambda: topk_kernel(work), a.reps, reset=lambda: work.copy_(logits)), 4)
        out["forward_only_ms"] = round(timed(lambda: model.last_hidden(ids), a.reps), 4)
        out["full_sampled_ratio"] = round(out["full_ms"] / out["sampled_uniform_ms"], 2)
        lines.append(out)
        print(json.dumps(out), flush=True)
        del model, logits, work
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as fh:
            fh.write("\n".join(json.dumps(o) for o in lines) + "\n")


if __name__ == "__main__":
    main()
