"""hipEvent times of Caser's convolution block (bsarec_caser_fwd + bsarec_caser_bwd: the training step between the embedding and
fc1) beside the torch formulation -- nn.Conv2d(1, n_v, (L, 1)) and, per height, nn.Conv2d(1, n_h, (h, d)) -> ReLU -> max_pool1d,
concatenated, forward and backward -- on the same GPU and from the same weights, in one process:

    python tools/caser_time.py                    # B = 256, L = 50, d = 64, n_v = 4, n_h = 8 and 16
    python tools/caser_time.py --once             # one forward + backward of ours per shape, nothing else (for a kernel trace)

Everything is allocated first; 20 warm-up and 100 timed iterations per shape, ours and torch's alternating call by call, an
event pair around each call.  Per shape one JSON line: the median / min / max milliseconds of both, ours split into forward and
backward, and the forward's achieved TFLOP/s from 2 B n_h d L (L + 1) (L + 2) / 6 FLOP against the 157 TFLOP/s fp32-MFMA peak.
If the torch formulation does not run on this build the line says so and carries ours alone."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
PEAK_TFLOPS = 157.0


def stats(ms):
    t = np.asarray(ms)
    return {"median": round(float(np.median(t)), 4), "min": round(float(t.min()), 4), "max": round(float(t.max()), 4)}


class TorchBlock(torch.nn.Module):
    def __init__(self, L, d, nh, nv):
        super().__init__()
        self.conv_v = torch.nn.Conv2d(1, nv, (L, 1))
        self.conv_h = torch.nn.ModuleList(torch.nn.Conv2d(1, nh, (i + 1, d)) for i in range(L))

    def forward(self, x):
        x = x.unsqueeze(1)
        out = [self.conv_v(x).reshape(x.shape[0], -1)]
        for conv in self.conv_h:
            c = torch.relu(conv(x).squeeze(3))
            out.append(torch.nn.functional.max_pool1d(c, c.shape[2]).squeeze(2))
        return torch.cat(out, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--seq_len", type=int, default=50)
    ap.add_argument("--hidden", type=int, default=64)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("caser_time: no GPU (there is nothing to measure on a CPU)")
    from bsarec_amd import _lib
    from bsarec_amd.caser import CaserConv
    lib = _lib.load()
    B, L, d, nv = a.batch, a.seq_len, a.hidden, 4
    for nh in (8, 16):
        torch.manual_seed(nh)
        conv = CaserConv(L, d, nh, nv).cuda()
        w = conv._flat
        cfg = _lib.CaserConfig(B, L, d, nh, nv)
        nb, nw, F = lib.bsarec_caser_workspace_bytes(cfg, 1), lib.bsarec_caser_weight_floats(cfg), conv.out_features
        g = torch.Generator(device="cuda").manual_seed(B + nh)
        x = torch.randn(B, L, d, device="cuda", generator=g)
        dz = torch.randn(B, F, device="cuda", generator=g)
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        z, dx, dw = torch.empty(B, F, device="cuda"), torch.empty(B, L, d, device="cuda"), torch.empty(nw, device="cuda")
        st = torch.cuda.current_stream().cuda_stream

        def ours_fwd():
            _lib.check(lib.bsarec_caser_fwd(cfg, x.data_ptr(), w.data_ptr(), 1, z.data_ptr(), ws.data_ptr(), nb, st), "fwd")

        def ours_bwd():
            _lib.check(lib.bsarec_caser_bwd(cfg, x.data_ptr(), w.data_ptr(), dz.data_ptr(), ws.data_ptr(), nb, dx.data_ptr(),
                                            dw.data_ptr(), st), "bwd")

        if a.once:
            ours_fwd(), ours_bwd()
            torch.cuda.synchronize()
            continue

        vendor, why = None, None
        try:
            block = TorchBlock(L, d, nh, nv).cuda()
            block.load_state_dict(conv.state_dict())
            tx = x.clone().requires_grad_(True)

            def vendor():
                for p in block.parameters():
                    p.grad = None
                tx.grad = None
                block(tx).backward(dz)
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
        flop = 2.0 * B * nh * d * L * (L + 1) * (L + 2) / 6
        tf = flop / (float(np.median(ms["fwd"])) * 1e-3) / 1e12
        line = {"B": B, "L": L, "d": d, "n_h": nh, "n_v": nv, "steps": a.steps,
                "ours_fwd_ms": stats(ms["fwd"]), "ours_bwd_ms": stats(ms["bwd"]), "ours_ms": stats(both),
                "fwd_gflop": round(flop / 1e9, 2), "fwd_tflops": round(tf, 2), "fwd_of_fp32_mfma_peak": round(tf / PEAK_TFLOPS, 3)}
        if vendor:
            line["torch_conv2d_maxpool_ms"] = stats(ms["vendor"])
            line["ours_over_torch"] = round(float(np.median(both) / np.median(ms["vendor"])), 3)
            line["z_max_abs_diff_vs_torch"] = float((block(x).detach() - z).abs().max())
        else:
            line["torch_conv2d_maxpool_ms"] = f"did not run: {why}"
        assert torch.isfinite(z).all() and torch.isfinite(dw).all() and torch.isfinite(dx).all()
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
