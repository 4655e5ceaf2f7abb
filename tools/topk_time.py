#!/usr/bin/env python3
"""Time bsarec_topk_seen (no seen mask) against torch.topk + a stable sort of the same rows, with hipEvents after warm-up.

    python tools/topk_time.py [--reps 20] [--shapes 256x3417x20,...]

One JSON line per (B, V, k): milliseconds per call of the HIP top-k and of torch (torch.topk of the k largest, then a stable
descending sort of those k values -- the library's tie order, NaN aside), and whether the two index lists agree.  The rows
are N(0, 1) floats, copied back before every call (the copy is outside the timed region).  BSAREC_LIB selects another build
of the library (an A/B of two kernels)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from bsarec_amd import _lib as Lb

SHAPES = [(256, 3417, 20), (256, 3417, 100), (256, 20034, 20), (256, 20034, 100), (256, 20034, 1024), (64, 100003, 100),
          (2048, 1_250_000, 20)]          # the last: one rank's shard of C5 (10,000,001 items over 8 GPUs), its 8 x 256 sequences


def timed(fn, reset, reps):
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2 * reps)]
    for _ in range(3):
        reset(); fn()
    total = 0.0
    for r in range(reps):
        reset()
        ev[2 * r].record(); fn(); ev[2 * r + 1].record()
    torch.cuda.synchronize()
    for r in range(reps):
        total += ev[2 * r].elapsed_time(ev[2 * r + 1])
    return total / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--shapes", default="", help="comma list of BxVxk (default: the issue's seven shapes)")
    a = ap.parse_args()
    shapes = [tuple(int(x) for x in s.split("x")) for s in a.shapes.split(",") if s] or SHAPES
    lib = Lb.load()
    st = torch.cuda.current_stream().cuda_stream
    for B, V, k in shapes:
        g = torch.Generator(device="cuda").manual_seed(V + k)
        src = torch.randn(B, V, device="cuda", generator=g)
        work = src.clone()
        idx = torch.empty(B, k, dtype=torch.int64, device="cuda")
        val = torch.empty(B, k, device="cuda")

        def hip():
            Lb.check(lib.bsarec_topk_seen(work.data_ptr(), V, B, V, None, None, None, k, idx.data_ptr(), val.data_ptr(), st),
                     "bsarec_topk_seen")

        out = {}

        def ref():
            v, i = torch.topk(work, k, dim=1)
            s = torch.sort(v, dim=1, descending=True, stable=True)
            out["i"] = torch.gather(i, 1, s.indices)

        reset = lambda: work.copy_(src)
        t_hip = timed(hip, reset, a.reps)
        t_ref = timed(ref, reset, a.reps)
        same = bool(torch.equal(idx, out["i"]))
        print(json.dumps({"B": B, "V": V, "k": k, "hip_ms": round(t_hip, 4), "torch_ms": round(t_ref, 4),
                          "speedup": round(t_ref / t_hip, 2), "same_indices": same,
                          "lib": os.path.basename(Lb.LIB_PATH)}), flush=True)
        del src, work


if __name__ == "__main__":
    main()
