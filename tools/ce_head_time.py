#!/usr/bin/env python3
"""The full-catalogue cross-entropy of a hidden state, torch (torch.matmul + F.cross_entropy + autograd, fp32) against HIP
(bsarec_ce_head_fwd / _bwd through the autograd node of BSARecModel.catalogue_ce): milliseconds per forward + backward of one
head call, peak memory above the inputs of one call, and milliseconds per calculate_loss + backward of DuoRec (us_x) at the C1
shape with and without --duorec_ce_head hip.

    python tools/ce_head_time.py [--reps 50] [--warmup 5] > profiles/ce_head_time.txt

One JSON line per measurement.  The two heads alternate within one process, call by call; each time is a hipEvent pair
around one call (the host's enqueue work included) followed by a synchronise, and the line gives the median and the min..max
spread.  h ~ N(0, 1), E ~ N(0, 1 / d), answers uniform.  Shapes of 10^9 scores and more run a fifth of the repetitions."""
import argparse
import json
import os
import sys
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from bsarec_amd import DuoRecModel, _lib
from bsarec_amd.model import _CatalogueCeFn

SHAPES = [(256, 3417, 64), (256, 100003, 64), (256, 1000003, 64), (2048, 1250001, 256)]
C1 = dict(item_size=3417, hidden_size=64, max_seq_length=50, num_hidden_layers=2, num_attention_heads=2, hidden_dropout_prob=0.5,
          attention_probs_dropout_prob=0.5, initializer_range=0.02, hidden_act="gelu", c=3, seed=1, batch_size=256)


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


def peak_above_inputs(fn, pools):
    """Peak of torch.cuda.max_memory_allocated over one call, above the level before it, in MB."""
    for p in pools:
        p.clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return round((torch.cuda.max_memory_allocated() - before) / 1e6, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    ce = torch.nn.functional.cross_entropy
    lib = _lib.load()
    for B, V, d in SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(B + V + d)
        h = torch.randn(B, d, device="cuda", generator=gen).requires_grad_(True)
        E = (torch.randn(V, d, device="cuda", generator=gen) / d ** 0.5).requires_grad_(True)
        ans = torch.randint(0, V, (B,), device="cuda", generator=gen)
        holder = types.SimpleNamespace(_ce_pool={})            # what the autograd node needs of a model: the workspace pool

        def torch_head():
            h.grad = E.grad = None
            loss = ce(torch.matmul(h, E.T), ans)
            loss.backward()
            return loss

        def hip_head():
            h.grad = E.grad = None
            loss = _CatalogueCeFn.apply(holder, h, E, ans)
            loss.backward()
            return loss

        big = B * V >= 10 ** 9
        reps, warmup = (max(a.reps // 5, 3), 2) if big else (a.reps, a.warmup)
        out = {"what": "head forward + backward", "B": B, "V": V, "d": d, "reps": reps,
               "workspace_MB": round(lib.bsarec_ce_head_workspace_bytes(B, V, d) / 1e6, 2),
               "logits_MB": round(B * V * 4 / 1e6, 2)}
        lt, lh = torch_head().item(), hip_head().item()
        out["loss_torch_hip"] = [round(lt, 6), round(lh, 6)]
        hip_head()
        dh_hip, dE_hip = h.grad.clone(), E.grad.clone()
        torch_head()
        out["dh_rel_l2_hip_vs_torch"] = float(f"{float((dh_hip - h.grad).norm() / h.grad.norm()):.2e}")
        out["dE_rel_l2_hip_vs_torch"] = float(f"{float((dE_hip - E.grad).norm() / E.grad.norm()):.2e}")
        del dh_hip, dE_hip
        h.grad = E.grad = None
        out["torch_peak_MB"] = peak_above_inputs(torch_head, [])
        h.grad = E.grad = None
        out["hip_peak_MB"] = peak_above_inputs(hip_head, [holder._ce_pool])
        report(out, alternate({"torch": torch_head, "hip": hip_head}, reps, warmup))
        del h, E, ans, holder
        torch.cuda.empty_cache()
    # the whole DuoRec step without the optimiser: three encoder passes, the CE over the catalogue, one InfoNCE term (us_x)
    rng = np.random.default_rng(0)
    B, L, V = C1["batch_size"], C1["max_seq_length"], C1["item_size"]
    ids = torch.from_numpy(rng.integers(1, V, (B, L))).cuda()
    sem = torch.from_numpy(rng.integers(1, V, (B, L))).cuda()
    ans = torch.from_numpy(rng.integers(1, V, (B,))).cuda()
    models = {k: DuoRecModel(argparse.Namespace(duorec_ce_head=k, ssl="us_x", sim="dot", tau=1.0, **C1)).cuda().train()
              for k in ("torch", "hip")}
    models["hip"].load_state_dict(models["torch"].state_dict())

    def step(mm):
        def run():
            mm.zero_grad()
            mm.calculate_loss(ids, ans, None, sem, None).backward()
        return run

    out = {"what": "DuoRec calculate_loss + backward (us_x, dot), C1 shape, by duorec_ce_head", "B": B, "L": L, "d": 64, "V": V}
    report(out, alternate({k: step(mm) for k, mm in models.items()}, a.reps, a.warmup))


if __name__ == "__main__":
    main()
