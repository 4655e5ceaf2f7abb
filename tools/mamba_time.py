"""hipEvent times of the selective state-space layer (bsarec_mamba_fwd + bsarec_mamba_bwd: one Mamba4Rec block's layer in a
training step) beside a torch restatement of the same layer on the same GPU, in one process:

    python tools/mamba_time.py                    # B = 256 and 1024, L = 50, d = 64, expand 2, d_state 16, d_conv 4, dt_rank 4

The baseline is NOT a vendor kernel: it is the layer written in torch ops with a Python loop over t
(tests/mamba_ref.py: torch_layer), forward and autograd backward -- what a user without this library would write first.
Everything is allocated first; 20 warm-up and 200 timed iterations per shape, ours and torch's alternating call by call, an
event pair around each call.  Per shape one JSON line: the median / min / max milliseconds of both, ours split into forward and
backward.  ``--ours_only`` leaves the baseline out (for a kernel trace of the library's launches alone)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def stats(ms):
    t = np.asarray(ms)
    return {"median": round(float(np.median(t)), 4), "min": round(float(t.min()), 4), "max": round(float(t.max()), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--seq_len", type=int, default=50)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--expand", type=int, default=2)
    ap.add_argument("--d_state", type=int, default=16)
    ap.add_argument("--d_conv", type=int, default=4)
    ap.add_argument("--ours_only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mamba_time: no GPU (there is nothing to measure on a CPU)")
    from bsarec_amd import _lib
    import mamba_ref as R
    lib = _lib.load()
    L, d = a.seq_len, a.hidden
    hyper = (a.expand, a.d_state, a.d_conv, R.dt_rank(d))
    for B in (256, 1024):
        cfg = _lib.MambaConfig(B, L, d, *hyper)
        nb, nw = lib.bsarec_mamba_workspace_bytes(cfg, 1), lib.bsarec_mamba_weight_floats(cfg)
        rng = np.random.default_rng(B)
        g = torch.Generator(device="cuda").manual_seed(B)
        x = torch.randn(B, L, d, device="cuda", generator=g)
        dy = torch.randn(B, L, d, device="cuda", generator=g)
        flat = R.random_weights(rng, d, *hyper)
        w = torch.from_numpy(flat).cuda()
        ids = torch.from_numpy(R.ragged_ids(rng, B, L)).cuda()
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        y, dx, dw = torch.empty(B, L, d, device="cuda"), torch.empty(B, L, d, device="cuda"), torch.empty(nw, device="cuda")
        st = torch.cuda.current_stream().cuda_stream

        def ours_fwd():
            _lib.check(lib.bsarec_mamba_fwd(cfg, x.data_ptr(), ids.data_ptr(), w.data_ptr(), 1, y.data_ptr(), ws.data_ptr(), nb, st), "fwd")

        def ours_bwd():
            _lib.check(lib.bsarec_mamba_bwd(cfg, x.data_ptr(), ids.data_ptr(), w.data_ptr(), dy.data_ptr(), ws.data_ptr(), nb,
                                          dx.data_ptr(), dw.data_ptr(), st), "bwd")

        base = None
        if not a.ours_only:
            tw = {k: torch.from_numpy(np.array(v)).cuda().requires_grad_(True) for k, v in R.split_weights(flat, d, *hyper).items()}
            tx = x.clone().requires_grad_(True)

            def base():
                for p in tw.values():
                    p.grad = None
                tx.grad = None
                ty = R.torch_layer(tx, ids, tw, hyper)
                ty.backward(dy)
                return ty

        def timed(fn):
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            fn()
            t1.record()
            torch.cuda.synchronize()
            return t0.elapsed_time(t1)

        for _ in range(a.warmup):
            ours_fwd(), ours_bwd()
            if base:
                base()
        torch.cuda.synchronize()
        ms = {"fwd": [], "bwd": [], "base": []}
        for _ in range(a.steps):
            ms["fwd"].append(timed(ours_fwd))
            ms["bwd"].append(timed(ours_bwd))
            if base:
                ms["base"].append(timed(base))
        both = np.asarray(ms["fwd"]) + np.asarray(ms["bwd"])
        line = {"B": B, "L": L, "d": d, "hyper": list(hyper), "steps": a.steps, "ours_fwd_ms": stats(ms["fwd"]), "ours_bwd_ms": stats(ms["bwd"]),
                "ours_ms": stats(both)}
        if base:
            ty = base()
            err = (torch.linalg.norm(ty.detach() - y) / torch.linalg.norm(y)).item()        # the two compute the same layer
            assert err < 1e-4, err
            line["torch_loop_ms"] = stats(ms["base"])
            line["ours_over_torch"] = round(float(np.median(both) / np.median(ms["base"])), 4)
            line["out_rel_l2_between_them"] = float(f"{err:.2e}")
        assert torch.isfinite(y).all() and torch.isfinite(dx).all() and torch.isfinite(dw).all()
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
