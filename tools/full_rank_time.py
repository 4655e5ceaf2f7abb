#!/usr/bin/env python3
"""Milliseconds per evaluation batch of the fused full-catalogue top-k (bsarec_topk_full) against the dense path (the B x V
fp32 score matrix, then bsarec_topk_seen), and the peak device memory each one adds.

    python tools/full_rank_time.py [--reps 20] [--shapes 256x1000003x64x20,...] [--only fused|dense]

One JSON line per (B, V, d, k).  The two paths alternate within one process, call by call; each time is a hipEvent pair
around one call after three warm-up calls, and the line gives the median and the min..max spread.  The dense matrix is
torch.mm(h, E.T) (the same GEMM shape as BSARecModel.full_logits).  h ~ N(0, 1), E ~ N(0, 0.1^2), 50 seen items per row.
Both paths return the same lists on these rows ("same": index lists equal)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bsarec_amd import _lib as Lb

SHAPES = [(256, 3417, 64, 20), (256, 100_003, 64, 20), (256, 100_003, 64, 100), (256, 1_000_003, 64, 20),
          (256, 1_000_003, 64, 100), (256, 1_000_003, 64, 1024)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="", help="comma list of BxVxdxk")
    ap.add_argument("--only", choices=("fused", "dense"), default=None, help="run one path only (for a profiler)")
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",") if s] or SHAPES
    lib = Lb.load()
    st = torch.cuda.current_stream().cuda_stream
    for B, V, d, k in shapes:
        g = torch.Generator(device="cuda").manual_seed(V + k)
        h = torch.randn(B, d, device="cuda", generator=g)
        E = torch.randn(V, d, device="cuda", generator=g) * 0.1
        n_seen = 50
        indices = torch.randint(0, V, (B * n_seen,), device="cuda", generator=g)
        indptr = torch.arange(0, B * n_seen + 1, n_seen, device="cuda", dtype=torch.int64)
        users = torch.arange(B, device="cuda", dtype=torch.int64)
        fi = torch.empty(B, k, dtype=torch.int64, device="cuda")
        di = torch.empty(B, k, dtype=torch.int64, device="cuda")
        nb = lib.bsarec_topk_full_workspace_bytes(B, V, d, k, 0)

        def fused():
            ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
            Lb.check(lib.bsarec_topk_full(h.data_ptr(), d, E.data_ptr(), B, V, d, users.data_ptr(), indptr.data_ptr(),
                                          indices.data_ptr(), k, 0, ws.data_ptr(), nb, fi.data_ptr(), None, st), "bsarec_topk_full")

        def dense():
            S = torch.mm(h, E.t())
            Lb.check(lib.bsarec_topk_seen(S.data_ptr(), V, B, V, users.data_ptr(), indptr.data_ptr(), indices.data_ptr(), k,
                                          di.data_ptr(), None, st), "bsarec_topk_seen")

        paths = {"fused": fused, "dense": dense}
        if a.only:
            paths = {a.only: paths[a.only]}
        times, peak = {p: [] for p in paths}, {}
        for p, fn in paths.items():
            torch.cuda.synchronize()
            base = torch.cuda.memory_allocated()
            torch.cuda.reset_peak_memory_stats()
            for _ in range(3):
                fn()
            torch.cuda.synchronize()
            peak[p] = (torch.cuda.max_memory_allocated() - base) / 2**20
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for _ in range(a.reps):
            for p, fn in paths.items():
                ev[0].record(); fn(); ev[1].record()
                torch.cuda.synchronize()
                times[p].append(ev[0].elapsed_time(ev[1]))
        out = {"B": B, "V": V, "d": d, "k": k}
        for p in paths:
            t = sorted(times[p])
            out[p + "_ms"] = round(t[len(t) // 2], 4)
            out[p + "_spread_ms"] = [round(t[0], 4), round(t[-1], 4)]
            out[p + "_peak_mb"] = round(peak[p], 1)
        if len(paths) == 2:
            out["speedup"] = round(out["dense_ms"] / out["fused_ms"], 2)
            out["same"] = bool(torch.equal(fi, di))
        print(json.dumps(out), flush=True)
        del h, E


if __name__ == "__main__":
    main()
