"""hipEvent times of one whole Caser optimisation step, three ways on the same GPU in one process:

    python tools/caser_step_time.py               # B = 256 and 1024, L = 50, d = 64, n_h = 16, n_v = 4, V = 3417, p = 0.5

  torch   caser_step = "torch": calculate_loss / backward / torch.optim.Adam over 2 L + 5 tensors, the default path
  eager   caser_step = "fused", caser_step_graph = False: bsarec_caser_train_step called per step
  graph   caser_step = "fused": the same call replayed from its captured graph

Three models of the same shape, everything allocated (and the graph captured) first; 20 warm-up and 200 timed steps, the three
paths alternating step by step, an event pair around each step.  Per shape one JSON line: median / min / max milliseconds of
each path and the ratios of the medians.  The host stays ahead of the device only as far as one step: an event pair is read
back after every step, so a path that is bound by launching from the host shows that cost.

    python tools/caser_step_time.py --user        # the personalised Caser (caser_user), U = 6040 users

  the three paths with the flag ON (the torch path is the torch-mode step of the personalised model) and, beside them,
  graph_off: the flag-off fused step of the same run, so that the cost of the user half's eight launches is visible."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seq_len", type=int, default=50)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--items", type=int, default=3417)
    ap.add_argument("--nh", type=int, default=16)
    ap.add_argument("--nv", type=int, default=4)
    ap.add_argument("--dropout", type=float, default=0.5)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 1024])
    ap.add_argument("--user", action="store_true", help="time the personalised Caser (caser_user) and the flag-off step beside it")
    ap.add_argument("--users", type=int, default=6040)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("caser_step_time: no GPU (there is nothing to measure on a CPU)")
    from bsarec_amd import CaserModel
    L, d, V = a.seq_len, a.hidden, a.items
    flag = dict(caser_user=True, num_users=a.users) if a.user else {}
    for B in a.batches:
        def model(**kw):
            torch.manual_seed(B)
            m = CaserModel(argparse.Namespace(item_size=V, hidden_size=d, max_seq_length=L, caser_nh=a.nh, caser_nv=a.nv,
                                              hidden_dropout_prob=a.dropout, initializer_range=0.02, lr=1e-3, adam_beta1=0.9,
                                              adam_beta2=0.999, weight_decay=0.0, **kw)).cuda()
            m.train()
            m.set_seed(42)
            return m
        mt, me, mg = model(**flag), model(caser_step="fused", caser_step_graph=False, **flag), model(caser_step="fused", **flag)
        g = torch.Generator(device="cuda").manual_seed(B)
        ids = torch.randint(1, V, (B, L), device="cuda", generator=g)
        pos = torch.randint(1, V, (B,), device="cuda", generator=g)
        neg = torch.randint(1, V, (B,), device="cuda", generator=g)
        users = torch.randint(0, a.users, (B,), device="cuda", generator=g) if a.user else None
        kw = dict(user_ids=users) if a.user else {}
        opt = torch.optim.Adam(mt.parameters(), lr=1e-3)

        def torch_step():
            loss = mt.calculate_loss(ids, pos, neg, **kw)
            opt.zero_grad()
            loss.backward()
            opt.step()
            return loss.detach()

        paths = {"torch": torch_step, "eager": lambda: me.train_step(ids, pos, neg, **kw),
                 "graph": lambda: mg.train_step(ids, pos, neg, **kw)}
        if a.user:
            m0 = model(caser_step="fused")
            paths["graph_off"] = lambda: m0.train_step(ids, pos, neg)

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
        line = {"B": B, "L": L, "d": d, "n_h": a.nh, "n_v": a.nv, "V": V, "dropout": a.dropout, "steps": a.steps,
                "optimiser_tensors": len(list(mt.parameters()))}
        if a.user:
            line["U"] = a.users
        line.update({f"{k}_ms": stats(v) for k, v in ms.items()})
        line["eager_over_torch"] = round(med["eager"] / med["torch"], 3)
        line["graph_over_torch"] = round(med["graph"] / med["torch"], 3)
        if a.user:
            line["graph_minus_graph_off_ms"] = round(med["graph"] - med["graph_off"], 4)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
