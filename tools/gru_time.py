"""hipEvent times of the GRU stack (bsarec_gru_fwd + bsarec_gru_bwd, last_only = 1: GRU4Rec's training step between the embedding
and the loss) beside torch's nn.GRU(bias=False) + nn.Linear forward and backward (the vendor path) on the same GPU, in one
process:

    python tools/gru_time.py                      # B = 256 and 1024, L = 50, d = H = 64, N = 1 and 2

Everything is allocated first; 20 warm-up and 200 timed iterations per shape, ours and torch's alternating call by call, an
event pair around each call.  Per shape one JSON line: the median / min / max milliseconds of both, ours split into forward and
backward, and ours per time step (the whole call over L: the recurrence is bound by the latency of one step times L).  If
torch's GRU does not run on this build the line says so and carries ours alone."""
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
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gru_time: no GPU (there is nothing to measure on a CPU)")
    from bsarec_amd import _lib
    lib = _lib.load()
    L, d, H = a.seq_len, a.hidden, a.hidden
    for B, N in ((256, 1), (256, 2), (1024, 1), (1024, 2)):
        cfg = _lib.GruConfig(B, L, d, H, N, d)
        nb, nw = lib.bsarec_gru_workspace_bytes(cfg, 1), lib.bsarec_gru_weight_floats(cfg)
        g = torch.Generator(device="cuda").manual_seed(B + N)
        x = torch.randn(B, L, d, device="cuda", generator=g)
        w = (torch.rand(nw, device="cuda", generator=g) * 2 - 1) / H ** 0.5
        dlast = torch.randn(B, d, device="cuda", generator=g)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        out, dx, dw = torch.empty(B, d, device="cuda"), torch.empty(B, L, d, device="cuda"), torch.empty(nw, device="cuda")
        st = torch.cuda.current_stream().cuda_stream

        def ours_fwd():
            _lib.check(lib.bsarec_gru_fwd(cfg, x.data_ptr(), w.data_ptr(), 1, 1, out.data_ptr(), ws.data_ptr(), nb, st), "fwd")

        def ours_bwd():
            _lib.check(lib.bsarec_gru_bwd(cfg, x.data_ptr(), w.data_ptr(), 1, dlast.data_ptr(), ws.data_ptr(), nb, dx.data_ptr(),
                                          dw.data_ptr(), st), "bwd")

        vendor, why = None, None
        try:
            gru = torch.nn.GRU(d, H, N, bias=False, batch_first=True).cuda()
            lin = torch.nn.Linear(H, d).cuda()
            tx = x.clone().requires_grad_(True)

            def vendor():
                for p in list(gru.parameters()) + list(lin.parameters()):
                    p.grad = None
                tx.grad = None
                lin(gru(tx)[0][:, -1]).backward(dlast)
            vendor()
            torch.cuda.synchronize()
        except Exception as e:                                # reported, not hidden: the line then carries ours alone
            vendor, why = None, f"{type(e).__name__}: {e}"

        def timed(fn):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1)

        for _ in range(a.warmup):
            ours_fwd(), ours_bwd()
            if vendor:
                vendor()
        torch.cuda.synchronize()
        ms = {"fwd": [], "bwd": [], "vendor": []}
        for _ in range(a.steps):
            ms["fwd"].append(timed(ours_fwd))
            ms["bwd"].append(timed(ours_bwd))
            if vendor:
                ms["vendor"].append(timed(vendor))
        both = np.asarray(ms["fwd"]) + np.asarray(ms["bwd"])
        line = {"B": B, "L": L, "d": d, "H": H, "N": N, "last_only": 1, "steps": a.steps,
                "ours_fwd_ms": stats(ms["fwd"]), "ours_bwd_ms": stats(ms["bwd"]), "ours_ms": stats(both),
                "ours_us_per_time_step": round(float(np.median(both)) * 1000 / L, 2)}
        if vendor:
            line["torch_gru_linear_ms"] = stats(ms["vendor"])
            line["ours_over_torch"] = round(float(np.median(both) / np.median(ms["vendor"])), 3)
        else:
            line["torch_gru_linear_ms"] = f"did not run: {why}"
        assert torch.isfinite(out).all() and torch.isfinite(dw).all()
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
