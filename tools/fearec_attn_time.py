"""ms per forward + backward of FEARec's autocorrelation attention: the HIP op (bsarec_amd.FeaAttention over bsarec_fea_attn_fwd /
_bwd) against a torch.fft restatement of the same math on the same GPU (rfft, band mask, irfft(n = L), channel mean, top-k,
softmax, a Python loop of rolls; autograd backward):

    python tools/fearec_attn_time.py                 # B = 256, L = 50, D = 64, bands (10, 26) and (0, 16), k = 3, training mode

Both sides run eagerly on one stream, warmed up.  A measurement is a window of `--reps` back-to-back calls of ONE side inside a
hipEvent pair, with a synchronise after it; the windows of the two sides alternate, `--steps` windows per side.  The outputs of the two sides are
compared first (same delays, out and dq to 1e-4 rel-L2), so that what is timed computes the same thing.  No threshold is attached:
the file records what was seen.  Writes profiles/fearec_attn_time.txt (one JSON line per band) unless --out says otherwise."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def fft_attention(q, k, v, lo, hi, topk, train):
    """The layer as it is usually written with torch.fft; the delays are chosen without gradient."""
    B, L, D = q.shape
    res = torch.fft.rfft(q, dim=1) * torch.conj(torch.fft.rfft(k, dim=1))
    box = torch.zeros_like(res)
    box[:, lo:hi] = res[:, lo:hi]
    m = torch.fft.irfft(box, n=L, dim=1).mean(-1)
    with torch.no_grad():
        if train:
            idx = torch.sort(-m.mean(0), stable=True).indices[:topk]
        else:
            idx = torch.sort(-m, dim=1, stable=True).indices[:, :topk]
    if train:
        p = torch.softmax(m[:, idx], dim=1)
        out = sum(p[:, i, None, None] * torch.roll(v, -int(s), dims=1) for i, s in enumerate(idx.tolist()))
    else:
        p = torch.softmax(m.gather(1, idx), dim=1)
        t = torch.arange(L, device=q.device)
        out = 0
        for i in range(topk):
            src = ((t[None, :] + idx[:, i:i + 1]) % L)[:, :, None].expand(B, L, D)
            out = out + p[:, i, None, None] * v.gather(1, src)
    return out, idx


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq_len", type=int, default=50)
    ap.add_argument("--width", type=int, default=64)
    ap.add_argument("--bands", default="10:26,0:16")
    ap.add_argument("--topk", type=int, default=3)
    ap.add_argument("--eval", action="store_true", help="evaluation mode (per-sequence delays) instead of training mode")
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fearec_attn_time.txt"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fearec_attn_time: needs the GPU (a CPU timing says nothing about it)")
    from bsarec_amd import FeaAttention, _lib
    B, L, D, train = a.batch, a.seq_len, a.width, not a.eval
    g = torch.Generator(device="cuda").manual_seed(0)
    q, k, v, w = (torch.randn(B, L, D, device="cuda", generator=g) for _ in range(4))
    lines = []
    for band in a.bands.split(","):
        lo, hi = (int(x) for x in band.split(":"))
        op = FeaAttention(L, D, lo, hi, a.topk).cuda().train(train)
        leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]

        def hip_call():
            for t in leaves:
                t.grad = None
            (op(*leaves) * w).sum().backward()

        def fft_call():
            for t in leaves:
                t.grad = None
            (fft_attention(*leaves, lo, hi, a.topk, train)[0] * w).sum().backward()

        # the two sides compute the same thing
        out_h = op(*leaves)
        (out_h * w).sum().backward()
        dq_h = leaves[0].grad.clone()
        for t in leaves:
            t.grad = None
        out_f, idx_f = fft_attention(*leaves, lo, hi, a.topk, train)
        (out_f * w).sum().backward()
        rel = lambda x, y: float((x - y).norm() / y.norm())
        agree = {"out": rel(out_h.detach(), out_f.detach()), "dq": rel(dq_h, leaves[0].grad)}
        assert agree["out"] <= 1e-4 and agree["dq"] <= 1e-4, agree
        for _ in range(a.warmup):
            hip_call()
            fft_call()
        torch.cuda.synchronize()
        ms = {"hip": [], "torch_fft": []}
        for _ in range(a.steps):
            for name, call in (("hip", hip_call), ("torch_fft", fft_call)):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                for _ in range(a.reps):
                    call()
                t1.record()
                torch.cuda.synchronize()
                ms[name].append(t0.elapsed_time(t1) / a.reps)
        rec = {"op": "fea_attn fwd+bwd", "mode": "train" if train else "eval", "B": B, "L": L, "D": D, "band": [lo, hi],
               "topk": a.topk, "steps": a.steps, "reps": a.reps, "agree_rel_l2": {n: float(f"{e:.2e}") for n, e in agree.items()},
               "device": torch.cuda.get_device_name(0), "source_sha16": _lib.source_sha16()}
        for name, t in ms.items():
            t = np.asarray(t)
            rec[name] = {"ms_median": round(float(np.median(t)), 4), "ms_min": round(float(t.min()), 4),
                         "ms_max": round(float(t.max()), 4)}
        rec["torch_fft_over_hip"] = round(rec["torch_fft"]["ms_median"] / rec["hip"]["ms_median"], 2)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write("# tools/fearec_attn_time.py: ms per forward + backward, eager calls including the autograd and launch overhead of\n"
                 "# both sides; medians of --steps windows of --reps calls of one side, the two sides' windows alternating.  No threshold is attached.\n")
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
