"""hipEvent times of one whole LRURec optimisation step, three ways on the same GPU in one process:

    python tools/lrurec_step_time.py              # B = 256 and 1024, L = 50, d = 64, N = 2, V = 3417, p = 0.5

  torch   lru_step = "torch": calculate_loss / backward / torch.optim.Adam, the default path
  eager   lru_step = "fused", lru_step_graph = False: bsarec_lrurec_train_step called per step
  graph   lru_step = "fused": the same call replayed from its captured graph

Three models of the same shape, everything allocated (and the graph captured) first; 20 warm-up and 200 timed steps, the three
paths alternating step by step, an event pair around each step.  Per shape one JSON line: median / min / max milliseconds of
each path, the ratios of the medians, and whether the replayed step's median lies below the torch step's minimum.  The host stays ahead of the device only as far as one step: an event pair is read
back after every step, so a path that is bound by launching from the host shows that cost."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def stats(ms):
    t = np.asarray(ms)
    return {"median": round(float(np.median(t)), 4), "min": round(float(t.min()), 4), "max": round(float(t.max()), 4)}


def main(model_name="LRURecModel", flag="lru_step", tool="lrurec_step_time"):
    """``model_name``: the block model to time; ``flag``: the name of its step flag; ``tool``: the name in the tool's messages
    (tools/mamba4rec_step_time.py passes its own)."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seq_len", type=int, default=50)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--layers", type=int, default=2)
    ap.add_argument("--items", type=int, default=3417)
    ap.add_argument("--dropout", type=float, default=0.5)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1024])
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit(f"{tool}: no GPU (there is nothing to measure on a CPU)")
    import bsarec_amd
    Model = getattr(bsarec_amd, model_name)
    L, d, V, N = a.seq_len, a.hidden, a.items, a.layers
    for B in a.batches:
        def model(**kw):
            torch.manual_seed(B + N)
            m = Model(argparse.Namespace(item_size=V, hidden_size=d, num_hidden_layers=N, max_seq_length=L,
                                         hidden_dropout_prob=a.dropout, initializer_range=0.02, lr=1e-3, adam_beta1=0.9,
                                         adam_beta2=0.999, weight_decay=0.0, **kw)).cuda()
            m.train()
            m.set_seed(42)
            return m
        mt, me, mg = model(), model(**{flag: "fused", flag + "_graph": False}), model(**{flag: "fused"})
        g = torch.Generator(device="cuda").manual_seed(B + N)
        ids = torch.randint(1, V, (B, L), device="cuda", generator=g)
        ans = torch.randint(1, V, (B,), device="cuda", generator=g)
        opt = torch.optim.Adam(mt.parameters(), lr=1e-3)

        def torch_step():
            loss = mt.calculate_loss(ids, ans)
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss.detach()

        paths = {"torch": torch_step, "eager": lambda: me.train_step(ids, ans), "graph": lambda: mg.train_step(ids, ans)}

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
        line = {"B": B, "L": L, "d": d, "N": N, "V": V, "dropout": a.dropout, "steps": a.steps}
        line.update({f"{k}_ms": stats(v) for k, v in ms.items()})
        line["eager_over_torch"] = round(med["eager"] / med["torch"], 3)
        line["graph_over_torch"] = round(med["graph"] / med["torch"], 3)
        line["graph_median_below_torch_min"] = bool(med["graph"] < min(ms["torch"]))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
