#!/usr/bin/env python3
"""DuoRec's contrastive head, torch (DuoRecModel.info_nce + F.cross_entropy + autograd) against HIP (bsarec_info_nce_fwd /
_bwd): milliseconds per forward + backward of one head call, errors of both against the fp64 restatement, and milliseconds
per calculate_loss + backward of the whole model (us_x) at the C1 shape under both heads.

    python tools/info_nce_time.py [--reps 200] [--warmup 20] > profiles/info_nce_time.txt

One JSON line per measurement.  The two heads alternate within one process, call by call; each time is a hipEvent pair
around one call (the host's enqueue work included: both heads are made of small launches) followed by a synchronise, and the
line gives the median and the min..max spread.  dot inputs ~ N(0, 0.3^2), cos inputs ~ N(0, 1), tau = 0.2."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import info_nce_ref as R
from bsarec_amd import DuoRecModel

SHAPES = [(256, 64), (1024, 64)]
C1 = dict(item_size=3417, hidden_size=64, max_seq_length=50, num_hidden_layers=2, num_attention_heads=2, hidden_dropout_prob=0.5,
          attention_probs_dropout_prob=0.5, initializer_range=0.02, hidden_act="gelu", c=3, seed=1, batch_size=256)


def model(head, **kw):
    return DuoRecModel(argparse.Namespace(duorec_head=head, **dict(C1, **kw))).cuda().train()


def alternate(fns, reps, warmup):
    """{name: sorted milliseconds per call}: the callables take turns, call by call."""
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
    out["torch_over_hip"] = round(out["torch_ms"] / out["hip_ms"], 2)
    print(json.dumps(out), flush=True)


def rel_l2(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b), 1e-30))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    ce = torch.nn.functional.cross_entropy
    m = model("hip")
    for B, d in SHAPES:
        for sim in ("dot", "cos"):
            m.sim, m.tau = sim, 0.2
            rng = np.random.default_rng(B + d)
            zi, zj = (rng.normal(0, 1.0 if sim == "cos" else 0.3, (B, d)).astype(np.float32) for _ in range(2))
            ti, tj = (torch.from_numpy(z).cuda().requires_grad_(True) for z in (zi, zj))

            def torch_head():
                ti.grad = tj.grad = None
                loss = ce(*m.info_nce(ti, tj, m.tau, B, sim))
                loss.backward()
                return loss

            def hip_head():
                ti.grad = tj.grad = None
                loss = m.info_nce_loss(ti, tj)
                loss.backward()
                return loss

            out = {"what": "head forward + backward", "B": B, "d": d, "sim": sim, "tau": m.tau}
            if B == 256:                                     # errors against fp64, g = 1
                rloss, _, rdi, rdj = R.info_nce(zi, zj, m.tau, sim, 1.0)
                for name, fn in (("torch", torch_head), ("hip", hip_head)):
                    loss = fn().item()
                    out[name + "_err"] = {"loss_rel": float(f"{abs(loss - rloss) / abs(rloss):.2e}"),
                                          "dz_i_rel_l2": float(f"{rel_l2(ti.grad.cpu().numpy(), rdi):.2e}"),
                                          "dz_j_rel_l2": float(f"{rel_l2(tj.grad.cpu().numpy(), rdj):.2e}")}
            report(out, alternate({"torch": torch_head, "hip": hip_head}, a.reps, a.warmup))
    # the whole DuoRec step without the optimiser: three encoder passes, the CE over the catalogue, one InfoNCE term (us_x)
    rng = np.random.default_rng(0)
    B, L, V = C1["batch_size"], C1["max_seq_length"], C1["item_size"]
    ids = torch.from_numpy(rng.integers(1, V, (B, L))).cuda()
    sem = torch.from_numpy(rng.integers(1, V, (B, L))).cuda()
    ans = torch.from_numpy(rng.integers(1, V, (B,))).cuda()
    for sim in ("dot", "cos"):
        models = {h: model(h, ssl="us_x", sim=sim, tau=1.0) for h in ("torch", "hip")}
        models["hip"].load_state_dict(models["torch"].state_dict())

        def step(mm):
            def run():
                mm.zero_grad()
                mm.calculate_loss(ids, ans, None, sem, None).backward()
            return run

        out = {"what": "DuoRec calculate_loss + backward (us_x), C1 shape", "B": B, "L": L, "d": 64, "V": V, "sim": sim}
        report(out, alternate({h: step(mm) for h, mm in models.items()}, a.reps, a.warmup))


if __name__ == "__main__":
    main()
