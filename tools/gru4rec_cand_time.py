"""hipEvent times of one whole GRU4Rec optimisation step with the heads over shared candidates, on the same GPU in one process:

    python tools/gru4rec_cand_time.py [--out FILE]   # B = 256 and 1024, L = 50, d = H = 64, N = 1 and 2, V = 3417, C = 2 B

  pair          gru_step = "fused", gru_loss = "bpr": the pairwise step replayed from its graph, the baseline
  torch:LOSS    gru_step = "torch" with the loss: calculate_loss (the head in torch ops) / backward / torch.optim.Adam
  eager:LOSS    gru_step = "fused", gru_step_graph = False: bsarec_gru4rec_cand_train_step called per step
  graph:LOSS    gru_step = "fused": the same call replayed from its captured graph

LOSS is ce, top1 and bpr_max, every one with gru_negatives = "in_batch+sampled".  Ten models of the same shape, everything
allocated (and the graphs captured) first; 20 warm-up and 200 timed steps, the paths alternating step by step, an event pair
around each step, read back after every step.  Per shape one line per path: median (min..max) in ms, and for the fused paths
the median minus the baseline's and over the torch path's."""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

LOSSES = ("ce", "top1", "bpr_max")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seq_len", type=int, default=50)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--items", type=int, default=3417)
    ap.add_argument("--dropout", type=float, default=0.5)
    ap.add_argument("--out", default=None, help="also write the lines to this file")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gru4rec_cand_time: no GPU (there is nothing to measure on a CPU)")
    from bsarec_amd import GRU4RecModel
    L, d, V = a.seq_len, a.hidden, a.items
    lines = []

    def say(text):
        print(text, flush=True)
        lines.append(text)

    for B, N in ((256, 1), (256, 2), (1024, 1), (1024, 2)):
        def model(**kw):
            torch.manual_seed(B + N)
            m = GRU4RecModel(argparse.Namespace(item_size=V, hidden_size=d, gru_hidden_size=d, num_hidden_layers=N, max_seq_length=L,
                                                hidden_dropout_prob=a.dropout, initializer_range=0.02, lr=1e-3, adam_beta1=0.9,
                                                adam_beta2=0.999, weight_decay=0.0, **kw)).cuda()
            m.train()
            m.set_seed(42)
            return m
        g = torch.Generator(device="cuda").manual_seed(B + N)
        ids = torch.randint(1, V, (B, L), device="cuda", generator=g)
        pos = torch.randint(1, V, (B,), device="cuda", generator=g)
        neg = torch.randint(1, V, (B,), device="cuda", generator=g)

        def torch_step(m, opt):
            def step():
                loss = m.calculate_loss(ids, pos, neg)
                opt.zero_grad()
                loss.backward()
                opt.step()
                return loss.detach()
            return step

        def fused_step(m):
            return lambda: m.train_step(ids, pos, neg)

        paths = {"pair": fused_step(model(gru_step="fused"))}
        for loss in LOSSES:
            kw = dict(gru_loss=loss, gru_negatives="in_batch+sampled")
            mt = model(**kw)
            paths[f"torch:{loss}"] = torch_step(mt, torch.optim.Adam(mt.parameters(), lr=1e-3))
            paths[f"eager:{loss}"] = fused_step(model(gru_step="fused", gru_step_graph=False, **kw))
            paths[f"graph:{loss}"] = fused_step(model(gru_step="fused", **kw))

        def timed(fn):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1)

        for _ in range(a.warmup):
            for fn in paths.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in paths}
        for _ in range(a.steps):
            for k, fn in paths.items():
                ms[k].append(timed(fn))
        last = {k: float(fn()) for k, fn in paths.items()}
        assert all(np.isfinite(v) for v in last.values()), last
        med = {k: float(np.median(v)) for k, v in ms.items()}
        say(f"B={B} L={L} d=H={d} N={N} V={V} C={2 * B} dropout={a.dropout} steps={a.steps}")
        for k, v in ms.items():
            text = f"  {k:14s} {med[k]:8.4f} ({min(v):.4f}..{max(v):.4f}) ms"
            kind, _, loss = k.partition(":")
            if kind in ("eager", "graph"):
                text += f"   - pair {med[k] - med['pair']:+.4f} ms   / torch {med[k] / med['torch:' + loss]:.3f}"
            say(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
