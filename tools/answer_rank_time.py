#!/usr/bin/env python3
"""Milliseconds per evaluation batch of the three full-ranking paths up to the one integer per row the metrics need: rank
(bsarec_answer_rank), fused (bsarec_topk_full, k = 20, then the answer looked up in the list) and dense (the B x V fp32 score
matrix, bsarec_topk_seen, k = 20, the same lookup).

    python tools/answer_rank_time.py [--reps 20] [--shapes 256x1000003x64,...] [--only rank|fused|dense]

One JSON line per (B, V, d).  The paths alternate within one process, call by call; each time is a hipEvent pair around one
call after three warm-up calls, and the line gives the median and the min..max spread.  h ~ N(0, 1), E ~ N(0, 0.1^2), 50 seen
items per row, answers uniform.  "same": wherever the fused list holds the answer it stands at the rank path's rank, and
nowhere else is that rank below k.  `--only rank` under `rocprofv3 --kernel-trace --stats` gives the per-kernel split."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bsarec_amd import _lib as Lb

SHAPES = [(256, 3417, 64), (256, 100_003, 64), (256, 1_000_003, 64)]
K = 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="", help="comma list of BxVxd")
    ap.add_argument("--only", choices=("rank", "fused", "dense"), default=None, help="run one path only (for a profiler)")
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",") if s] or SHAPES
    lib = Lb.load()
    st = torch.cuda.current_stream().cuda_stream
    for B, V, d in shapes:
        g = torch.Generator(device="cuda").manual_seed(V)
        h = torch.randn(B, d, device="cuda", generator=g)
        E = torch.randn(V, d, device="cuda", generator=g) * 0.1
        n_seen = 50
        indices = torch.randint(0, V, (B * n_seen,), device="cuda", generator=g)
        indptr = torch.arange(0, B * n_seen + 1, n_seen, device="cuda", dtype=torch.int64)
        users = torch.arange(B, device="cuda", dtype=torch.int64)
        answers = torch.randint(0, V, (B,), device="cuda", generator=g)
        answers[::4] = torch.topk(torch.mm(h[::4], E.t()), 5, dim=1).indices[:, 4]       # a quarter of them inside the lists
        fi = torch.empty(B, K, dtype=torch.int64, device="cuda")
        di = torch.empty(B, K, dtype=torch.int64, device="cuda")
        rank = torch.empty(B, dtype=torch.int32, device="cuda")
        score = torch.empty(B, dtype=torch.float32, device="cuda")
        nb = lib.bsarec_topk_full_workspace_bytes(B, V, d, K, 0)
        hits = {}

        def by_rank():
            Lb.check(lib.bsarec_answer_rank(h.data_ptr(), d, E.data_ptr(), B, V, d, users.data_ptr(), indptr.data_ptr(),
                                            indices.data_ptr(), answers.data_ptr(), rank.data_ptr(), score.data_ptr(), st),
                     "bsarec_answer_rank")

        def fused():
            ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
            Lb.check(lib.bsarec_topk_full(h.data_ptr(), d, E.data_ptr(), B, V, d, users.data_ptr(), indptr.data_ptr(),
                                          indices.data_ptr(), K, 0, ws.data_ptr(), nb, fi.data_ptr(), None, st), "bsarec_topk_full")
            hits["fused"] = fi == answers.view(-1, 1)

        def dense():
            S = torch.mm(h, E.t())
            Lb.check(lib.bsarec_topk_seen(S.data_ptr(), V, B, V, users.data_ptr(), indptr.data_ptr(), indices.data_ptr(), K,
                                          di.data_ptr(), None, st), "bsarec_topk_seen")
            hits["dense"] = di == answers.view(-1, 1)

        paths = {"rank": by_rank, "fused": fused, "dense": dense}
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
        out = {"B": B, "V": V, "d": d, "k": K}
        for p in paths:
            t = sorted(times[p])
            out[p + "_ms"] = round(t[len(t) // 2], 4)
            out[p + "_spread_ms"] = [round(t[0], 4), round(t[-1], 4)]
            out[p + "_peak_mb"] = round(peak[p], 1)
        if not a.only:
            out["fused_over_rank"] = round(out["fused_ms"] / out["rank_ms"], 2)
            out["dense_over_rank"] = round(out["dense_ms"] / out["rank_ms"], 2)
            hit = hits["fused"]
            pos = torch.where(hit.any(1), hit.int().argmax(1), torch.full((B,), -1, device="cuda"))
            r = rank.long()
            out["same"] = bool(((pos >= 0) == (r < K)).all() and (pos[pos >= 0] == r[pos >= 0]).all())
            out["answers_in_lists"] = int((pos >= 0).sum())
        print(json.dumps(out), flush=True)
        del h, E


if __name__ == "__main__":
    main()
