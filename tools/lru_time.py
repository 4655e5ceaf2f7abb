"""hipEvent times of the linear recurrent unit layer (bsarec_lru_fwd + bsarec_lru_bwd: one LRURec block's recurrent layer in a
training step) beside a torch restatement of the same layer on the same GPU, in one process:

    python tools/lru_time.py                      # B = 256 and 1024, L = 50, d = 64

The baseline is NOT a vendor kernel: it is the layer written with torch complex tensors and a Python loop over t
(tests/lru_ref.py: torch_complex_layer), forward and autograd backward -- what a user without this library would write first.
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
    ap.add_argument("--ours_only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lru_time: no GPU (there is nothing to measure on a CPU)")
    from bsarec_amd import _lib
    import lru_ref as R
    lib = _lib.load()
    L, d = a.seq_len, a.hidden
    for B in (256, 1024):
        cfg = _lib.LruConfig(B, L, d)
        nb, nw = lib.bsarec_lru_workspace_bytes(cfg, 1), lib.bsarec_lru_weight_floats(cfg)
        rng = np.random.default_rng(B)
        g = torch.Generator(device="cuda").manual_seed(B)
        x = torch.randn(B, L, d, device="cuda", generator=g)
        dy = torch.randn(B, L, d, device="cuda", generator=g)
        flat = R.random_weights(rng, d)
        w = torch.from_numpy(flat).cuda()
        ids = torch.from_numpy(R.ragged_ids(rng, B, L)).cuda()
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        y, dx, dw = torch.empty(B, L, d, device="cuda"), torch.empty(B, L, d, device="cuda"), torch.empty(nw, device="cuda")
        st = torch.cuda.current_stream().cuda_stream

        def ours_fwd():
            _lib.check(lib.bsarec_lru_fwd(cfg, x.data_ptr(), ids.data_ptr(), w.data_ptr(), 1, y.data_ptr(), ws.data_ptr(), nb, st), "fwd")

        def ours_bwd():
            _lib.check(lib.bsarec_lru_bwd(cfg, x.data_ptr(), ids.data_ptr(), w.data_ptr(), dy.data_ptr(), ws.data_ptr(), nb,
                                          dx.data_ptr(), dw.data_ptr(), st), "bwd")

        base = None
        if not a.ours_only:
            tw = {k: torch.from_numpy(np.array(v)).cuda().requires_grad_(True) for k, v in R.split_weights(flat, d).items()}
            tx = x.clone().requires_grad_(True)

            def base():
                for p in tw.values():
                    p.grad = None
                tx.grad = None
                ty = R.torch_complex_layer(tx, ids, tw)
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
        line = {"B": B, "L": L, "d": d, "steps": a.steps, "ours_fwd_ms": stats(ms["fwd"]), "ours_bwd_ms": stats(ms["bwd"]),
                "ours_ms": stats(both)}
        if base:
            ty = base()
            err = (torch.linalg.norm(ty.detach() - y) / torch.linalg.norm(y)).item()        # the two compute the same layer
            assert err < 1e-4, err
            line["torch_complex_loop_ms"] = stats(ms["base"])
            line["ours_over_torch"] = round(float(np.median(both) / np.median(ms["base"])), 4)
            line["y_rel_l2_between_them"] = float(f"{err:.2e}")
        assert torch.isfinite(y).all() and torch.isfinite(dx).all() and torch.isfinite(dw).all()
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
