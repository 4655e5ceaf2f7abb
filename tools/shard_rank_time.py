#!/usr/bin/env python3
"""Milliseconds per evaluation batch of ONE rank of the catalogue-sharded evaluation at the shard's own shape, fused
(bsarec_topk_full_range over the owned rows) against dense (bsarec_shard_logits into the partial logits [Bg, Vs], the torch
scatter that zeroes the seen items, bsarec_topk_seen), and the peak device memory each one adds.

    python tools/shard_rank_time.py [--reps 20] [--shapes 2048x1250001x256x20,...] [--base 3750003] [--only fused|dense]

One process, one GPU, no collectives: what one rank of ShardedCatalogue.topk runs between its all-gathers; the
default shape is one shard of C5 (V = 10 M over 8 ranks, d = 256, 8 x 256 sequences).  One JSON line per (Bg, Vs, d, k).  The
two paths alternate call by call; each time is a hipEvent pair around one call after three warm-up calls, and the line gives the
median and the min..max spread.  The dense path's logits are allocated once, as ShardedCatalogue keeps them; the peak counts
them.  h ~ N(0, 1), E ~ N(0, 0.05^2), 50 global seen ids per row, half of them inside the range.  "same": the two index lists
agree (bsarec_shard_logits sums in another order than the fmaf chain, so near ties may swap: the fraction is printed)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bsarec_amd import _lib as Lb

SHAPES = [(2048, 1_250_001, 256, 20), (2048, 1_250_001, 256, 100)]
N_SEEN = 50


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="", help="comma list of BgxVsxdxk")
    ap.add_argument("--base", type=int, default=-1, help="column base of the range (default: 3 * Vs)")
    ap.add_argument("--only", choices=("fused", "dense"), default=None, help="run one path only (for a profiler)")
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",") if s] or SHAPES
    lib = Lb.load()
    st = torch.cuda.current_stream().cuda_stream
    for Bg, Vs, d, k in shapes:
        base = a.base if a.base >= 0 else 3 * Vs
        g = torch.Generator(device="cuda").manual_seed(Vs + k)
        h = torch.randn(Bg, d, device="cuda", generator=g)
        E = torch.randn(Vs, d, device="cuda", generator=g) * 0.05
        inside = base + torch.randint(0, Vs, (Bg, N_SEEN // 2), device="cuda", generator=g)
        outside = torch.randint(0, base, (Bg, N_SEEN - N_SEEN // 2), device="cuda", generator=g) if base else \
            base + Vs + torch.randint(0, Vs, (Bg, N_SEEN - N_SEEN // 2), device="cuda", generator=g)
        seen = torch.cat([inside, outside], 1).contiguous()                 # [Bg, S] global ids, as the all-gathered seen lists
        indptr = torch.arange(Bg + 1, device="cuda", dtype=torch.int64) * N_SEEN
        users = torch.arange(Bg, device="cuda", dtype=torch.int64)
        fi = torch.empty(Bg, k, dtype=torch.int64, device="cuda")
        di = torch.empty(Bg, k, dtype=torch.int64, device="cuda")
        nb = lib.bsarec_topk_full_workspace_bytes(Bg, Vs, d, k, 0)
        ld = (Vs + 3) // 4 * 4
        buf = {}

        def fused():
            if "ws" not in buf:                                             # cached per (Bg, k), as ShardedCatalogue does
                buf["ws"] = torch.empty(nb, dtype=torch.uint8, device="cuda")
            Lb.check(lib.bsarec_topk_full_range(h.data_ptr(), d, E.data_ptr(), Bg, Vs, base, d, users.data_ptr(), indptr.data_ptr(),
                                                seen.data_ptr(), k, 0, buf["ws"].data_ptr(), nb, fi.data_ptr(), None, st),
                     "bsarec_topk_full_range")

        def dense():
            if "logits" not in buf:
                buf["logits"] = torch.zeros(Bg, ld, dtype=torch.float32, device="cuda")
            logits = buf["logits"]
            Lb.check(lib.bsarec_shard_logits(h.data_ptr(), d, Bg, E.data_ptr(), Vs, d, logits.data_ptr(), ld, st), "bsarec_shard_logits")
            scores = logits[:, :Vs]
            loc = seen - base
            ok = (seen >= 0) & (loc >= 0) & (loc < Vs)
            rows = torch.arange(Bg, device="cuda").view(Bg, 1).expand(Bg, N_SEEN)
            scores[rows[ok], loc[ok]] = 0.0
            Lb.check(lib.bsarec_topk_seen(scores.data_ptr(), ld, Bg, Vs, None, None, None, k, di.data_ptr(), None, st), "bsarec_topk_seen")

        paths = {"fused": fused, "dense": dense}
        if a.only:
            paths = {a.only: paths[a.only]}
        times, peak = {p: [] for p in paths}, {}
        for p, fn in paths.items():
            torch.cuda.synchronize()
            start = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            peak[p] = (torch.cuda.max_memory_allocated() - start) / 2**20
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for _ in range(a.reps):
            for p, fn in paths.items():
                ev[0].record(); fn(); ev[1].record()
                torch.cuda.synchronize()
                times[p].append(ev[0].elapsed_time(ev[1]))
        out = {"Bg": Bg, "Vs": Vs, "d": d, "k": k, "base": base}
        for p in paths:
            t = sorted(times[p])
            out[p + "_ms"] = round(t[len(t) // 2], 4)
            out[p + "_spread_ms"] = [round(t[0], 4), round(t[-1], 4)]
            out[p + "_peak_mb"] = round(peak[p], 1)
        if len(paths) == 2:
            out["dense_over_fused"] = round(out["dense_ms"] / out["fused_ms"], 2)
            out["same"] = round(float((fi == di + base).float().mean()), 6)
        print(json.dumps(out), flush=True)
        del h, E, buf


if __name__ == "__main__":
    main()
