#!/usr/bin/env python3
"""Per-workgroup record of the weight-gradient launch (dw_direct_kernel), C1 shape: where each workgroup ran, when it
started and ended.  Needs a library built with -DBSAREC_DW_STAMPS (the default build has no such code):

    hipcc <flags of bsarec_amd/build.py> -DBSAREC_DW_STAMPS bsarec_amd/csrc/bsarec_hip.hip -o /tmp/libstamps.so
    BSAREC_LIB=/tmp/libstamps.so python tools/dw_stamps.py [--splits N] [--out FILE]
"""
import argparse, ctypes as C, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap = argparse.ArgumentParser()
ap.add_argument("--splits", type=int, default=0)
ap.add_argument("--out", default=None, help="also write one line per workgroup here")
o = ap.parse_args()
if o.splits:
    os.environ["BSAREC_SPLITS"] = str(o.splits)
import numpy as np, torch
from bsarec_amd import BSARecModel, _lib as Lb
import bench
a = argparse.Namespace(item_size=3417, hidden=64, seq_len=50, batch=256, layers=2, heads=2)
m = BSARecModel(bench.model_args(a)).cuda(); m.train(); m.configure_adam()
ids = torch.randint(1, 3417, (256, 50), device="cuda"); ids[:, :20] = 0
ans = torch.randint(1, 3417, (256,), device="cuda")
lib = Lb.load()
fn = C.CDLL(Lb.LIB_PATH).bsarec_debug_dw_stamps          # AttributeError: not a -DBSAREC_DW_STAMPS build
fn.restype = C.c_int; fn.argtypes = [C.c_void_p, C.c_int]
for _ in range(5): m.train_step(ids, ans)
torch.cuda.synchronize()
N = 2048
raw = np.zeros((N, 8), dtype=np.int64)
assert fn(raw.ctypes.data, N) == 0
blk = np.nonzero(raw[:, 1] > 0)[0]
raw = raw[blk]
t0 = raw[:, 0].min()
beg, end = (raw[:, 0] - t0) * 0.01, (raw[:, 1] - t0) * 0.01          # 100 MHz clock -> us
hw, xcc, kind = raw[:, 2] & 0xFFFFFFFF, (raw[:, 2] >> 32) & 0xF, raw[:, 3]
cu = (xcc << 8) | (((hw >> 13) & 7) << 5) | (((hw >> 12) & 1) << 4) | ((hw >> 8) & 15)      # (xcc, se, sh, cu)
names = ["big", "small", "scatter", "tick", "empty"]
print(f"{len(raw)} workgroups, launch spans {end.max():.2f} us on {len(set(cu))} CUs")
for k, nm in enumerate(names):
    s = kind == k
    if s.any():
        print(f"  {nm:8s} n={s.sum():4d} start {beg[s].min():6.2f} .. {beg[s].max():6.2f}  end {end[s].min():6.2f} .. {end[s].max():6.2f}"
              f"  mean length {np.mean(end[s] - beg[s]):6.2f} us")
big = kind == 0
# wave 0 of the product workgroups: entry -> operands known -> k loop done -> past the barrier -> slab stored
for k in (0, 1):
    s = (kind == k) & (raw[:, 4] > 0)
    if s.any():
        ph = np.stack([raw[s, 0], raw[s, 4], raw[s, 5], raw[s, 6], raw[s, 1]], 1)
        d = np.diff(ph, axis=1) * 0.01
        print(f"  {names[k]:8s} phases (us, mean): set-up {d[:, 0].mean():.2f}  k loop {d[:, 1].mean():.2f}  barrier {d[:, 2].mean():.2f}"
              f"  reduce + store {d[:, 3].mean():.2f}")
# big workgroups that overlap in time on one CU: how many CUs ever hold 2 (or more) at once
per_cu = {}
for c, b, e in zip(cu[big], beg[big], end[big]):
    per_cu.setdefault(int(c), []).append((b, e))
hist = {}
for c, iv in per_cu.items():
    peak = max(sum(1 for (b2, e2) in iv if b2 <= b < e2) for (b, _) in iv)
    hist[peak] = hist.get(peak, 0) + 1
hist[0] = len(set(cu)) - len(per_cu)
print("  CUs by peak number of co-resident big workgroups:", dict(sorted(hist.items())))
for peak in sorted(set(hist) - {0}):
    sel = [c for c, iv in per_cu.items() if max(sum(1 for (b2, e2) in iv if b2 <= b < e2) for (b, _) in iv) == peak]
    ends = [max(e for _, e in per_cu[c]) for c in sel]
    lens = [e - b for c in sel for b, e in per_cu[c]]
    print(f"    peak {peak}: last big end {np.mean(ends):6.2f} us mean, {max(ends):6.2f} max; big workgroup length {np.mean(lens):6.2f} us mean")
if o.out:
    with open(o.out, "w") as f:
        f.write("# block kind xcc se sh cu start_us end_us\n")
        for i in np.argsort(beg):
            f.write(f"{blk[i]} {names[kind[i]]} {xcc[i]} {(hw[i] >> 13) & 7} {(hw[i] >> 12) & 1} {(hw[i] >> 8) & 15} {beg[i]:.2f} {end[i]:.2f}\n")
