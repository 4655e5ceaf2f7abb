"""The GRU stack kernels on the GPU (bsarec_gru_fwd / bsarec_gru_bwd, csrc/gru.h) through ctypes against the fp64 restatement
(gru_ref): every shape with last_only 0 and 1, row independence, determinism, graph capture, saturated gates, train = 0.
Inputs are N(0, 1) rounded to fp32, weights U(-1/sqrt(H), 1/sqrt(H)).  Gates: the fused-path gates of test_gpu_parity.py --
outputs <= 2e-5 rel-L2, every gradient tensor <= 2e-4 rel-L2."""
import functools

import numpy as np
import pytest

from conftest import rel_l2
import gru_ref as R

pytestmark = pytest.mark.gpu
OUT_GATE, GRAD_GATE = 2e-5, 2e-4

SHAPES = [(1, 1, 4, 32, 1, 0), (2, 2, 64, 64, 1, 64), (31, 50, 64, 64, 2, 64), (32, 50, 64, 64, 2, 64), (33, 50, 64, 64, 2, 64),
          (65, 20, 100, 96, 1, 100), (17, 50, 256, 128, 2, 256), (5, 256, 64, 128, 4, 64), (256, 50, 64, 64, 1, 64),
          (3, 255, 8, 32, 3, 4)]
SAT = (33, 50, 64, 64, 2, 64)


class Call:
    """Static buffers of one shape and the two entries on the current stream; outputs start as NaN."""

    def __init__(self, shape, x, flat, dout, last_only, train=1):
        import torch
        from bsarec_amd import _lib
        self.lib, self._lib = _lib.load(), _lib
        B, L, I, H, N, O = shape
        self.cfg = _lib.GruConfig(B, L, I, H, N, O)
        self.nb = self.lib.bsarec_gru_workspace_bytes(self.cfg, train)
        assert self.nb > 0 and self.lib.bsarec_gru_weight_floats(self.cfg) == flat.size
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device="cuda")
        self.x, self.flat = torch.from_numpy(x).cuda(), torch.from_numpy(flat).cuda()
        self.dout = None if dout is None else torch.from_numpy(np.ascontiguousarray(dout, dtype=np.float32)).cuda()
        W = O or H
        self.out = torch.empty((B, W) if last_only else (B, L, W), device="cuda")
        self.dx, self.dw = torch.empty(B, L, I, device="cuda"), torch.empty(flat.size, device="cuda")
        self.last_only, self.train = int(last_only), int(train)
        self.poison()

    def poison(self):
        for t in (self.out, self.dx, self.dw):
            t.fill_(float("nan"))

    def launch(self, backward=True):
        import torch
        st = torch.cuda.current_stream().cuda_stream
        self._lib.check(self.lib.bsarec_gru_fwd(self.cfg, self.x.data_ptr(), self.flat.data_ptr(), self.train, self.last_only,
                                                self.out.data_ptr(), self.ws.data_ptr(), self.nb, st), "bsarec_gru_fwd")
        if backward and self.dout is not None:
            self._lib.check(self.lib.bsarec_gru_bwd(self.cfg, self.x.data_ptr(), self.flat.data_ptr(), self.last_only,
                                                    self.dout.data_ptr(), self.ws.data_ptr(), self.nb, self.dx.data_ptr(),
                                                    self.dw.data_ptr(), st), "bsarec_gru_bwd")
        return self

    def results(self):
        return self.out.cpu().numpy(), self.dx.cpu().numpy(), self.dw.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(shape, scale=1.0):
    """fp32-rounded inputs and the fp64 reference of both forms, computed once per case."""
    B, L, I, H, N, O = shape
    rng = np.random.default_rng(sum(p * v for p, v in zip((7, 11, 13, 17, 19, 23), shape)))
    x = (rng.normal(0, 1, (B, L, I)) * scale).astype(np.float32)
    flat = R.random_weights(rng, I, H, N, O, scale)
    dout = rng.normal(0, 1, (B, L, O or H)).astype(np.float32)
    dlast = rng.normal(0, 1, (B, O or H)).astype(np.float32)
    out, cache = R.forward(x, flat, H, N, O)
    return x, flat, dout, dlast, out, R.backward(cache, dout), R.backward(cache, R.last_only_dout(dlast, L))


def _grad_errors(shape, got_dx, got_dw, ref_dx, ref_dw):
    B, L, I, H, N, O = shape
    errs = {"dx": rel_l2(got_dx, ref_dx)}
    g, r = R.split_weights(got_dw, I, H, N, O), R.split_weights(ref_dw, I, H, N, O)
    for k in r:
        errs[k] = rel_l2(g[k], r[k])
    return errs


@pytest.mark.parametrize("last_only", [0, 1])
@pytest.mark.parametrize("shape", SHAPES, ids=["-".join(map(str, s)) for s in SHAPES])
def test_kernel_vs_fp64_reference(shape, last_only):
    B, L, I, H, N, O = shape
    x, flat, dout, dlast, rout, rfull, rlast = _case(shape)
    out, dx, dw = Call(shape, x, flat, dlast if last_only else dout, last_only).launch().results()
    assert np.isfinite(out).all() and np.isfinite(dx).all() and np.isfinite(dw).all()      # every float overwritten
    e_out = rel_l2(out, rout[:, L - 1] if last_only else rout)
    errs = _grad_errors(shape, dx, dw, *(rlast if last_only else rfull))
    print(f"gru {shape} last_only={last_only}: out {e_out:.2e} " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert e_out <= OUT_GATE
    if last_only:
        # row L - 1 of the full output, bit for bit; the gradients of the full entry fed a dout that is zero except at L - 1
        fout, fdx, fdw = Call(shape, x, flat, R.last_only_dout(dlast, L), 0).launch().results()
        assert np.array_equal(out, fout[:, L - 1])
        for k, v in _grad_errors(shape, dx, dw, fdx, fdw).items():
            assert v <= GRAD_GATE, (k, v)
    if L == 1:
        g = R.split_weights(dw, I, H, N, O)
        assert not any(g[f"weight_hh_l{k}"].any() for k in range(N))      # h_{-1} = 0: exactly zero
    for k, v in errs.items():
        assert v <= GRAD_GATE, (k, v)


def test_row_independence():
    """Sequence 7 of the (33, 50, 64, 64, 2, 64) case, run alone as B = 1, gives the same forward bits."""
    shape = (33, 50, 64, 64, 2, 64)
    x, flat = _case(shape)[:2]
    full = Call(shape, x, flat, None, 0).launch().results()[0]
    alone = Call((1,) + shape[1:], np.ascontiguousarray(x[7:8]), flat, None, 0).launch().results()[0]
    assert np.array_equal(full[7], alone[0])
    last = Call((1,) + shape[1:], np.ascontiguousarray(x[7:8]), flat, None, 1).launch().results()[0]
    assert np.array_equal(full[7, -1], last[0])


@pytest.mark.parametrize("shape", [(33, 50, 64, 64, 2, 64), (65, 20, 100, 96, 1, 100)], ids=["33-50-64-64-2-64", "65-20-100-96-1-100"])
def test_determinism_and_train0(shape):
    x, flat, dout = _case(shape)[:3]
    a = Call(shape, x, flat, dout, 0).launch().results()
    b = Call(shape, x, flat, dout, 0).launch().results()
    for u, v in zip(a, b):
        assert np.isfinite(u).all() and np.array_equal(u, v)
    c = Call(shape, x, flat, dout, 0)
    c.launch()
    c.poison()
    again = c.launch().results()                      # the same workspace a second time
    for u, v in zip(a, again):
        assert np.array_equal(u, v)
    for last_only in (0, 1):
        ev = Call(shape, x, flat, None, last_only, train=0).launch().results()[0]
        tr = Call(shape, x, flat, None, last_only, train=1).launch().results()[0]
        assert np.array_equal(ev, tr)
    assert np.array_equal(tr, a[0][:, -1])


@pytest.mark.parametrize("last_only", [0, 1])
def test_graph_capture(last_only):
    """Forward and backward captured once and replayed three times give the bits of the eager call."""
    import torch
    shape = (33, 50, 64, 64, 2, 64)
    x, flat, dout, dlast = _case(shape)[:4]
    c = Call(shape, x, flat, dlast if last_only else dout, last_only)
    eager = c.launch().results()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c.launch()
    for _ in range(3):
        c.poison()
        graph.replay()
        torch.cuda.synchronize()
        for u, v in zip(eager, c.results()):
            assert np.array_equal(u, v)


def test_saturated_gates():
    """Weights x 8 and inputs x 8: everything finite, |h| <= 1, and rel-L2 errors against fp64 at most 8 x the error torch's CPU
    fp32 nn.GRU + nn.Linear make on the same inputs (computed here; the margin covers other exp / tanh and sum orders)."""
    import torch
    shape = SAT
    B, L, I, H, N, O = shape
    x, flat, dout, dlast, rout, rfull, rlast = _case(shape, 8.0)
    out, dx, dw = Call(shape, x, flat, dout, 0).launch().results()
    assert np.isfinite(out).all() and np.isfinite(dx).all() and np.isfinite(dw).all()
    nw = sum(int(np.prod(s)) for _, s in R.weight_shapes(I, H, N, 0))
    h = Call((B, L, I, H, N, 0), x, np.ascontiguousarray(flat[:nw]), None, 0).launch().results()[0]
    assert np.isfinite(h).all() and np.abs(h).max() <= 1.0

    w = R.split_weights(flat, I, H, N, O)
    gru, lin = torch.nn.GRU(I, H, N, bias=False, batch_first=True), torch.nn.Linear(H, O)
    with torch.no_grad():
        for k in range(N):
            getattr(gru, f"weight_ih_l{k}").copy_(torch.from_numpy(w[f"weight_ih_l{k}"]))
            getattr(gru, f"weight_hh_l{k}").copy_(torch.from_numpy(w[f"weight_hh_l{k}"]))
        lin.weight.copy_(torch.from_numpy(w["out_weight"]))
        lin.bias.copy_(torch.from_numpy(w["out_bias"]))
    tx = torch.from_numpy(x).requires_grad_(True)
    tout = lin(gru(tx)[0])
    tout.backward(torch.from_numpy(dout))
    tg = {f"weight_ih_l{k}": getattr(gru, f"weight_ih_l{k}").grad.numpy() for k in range(N)}
    tg.update({f"weight_hh_l{k}": getattr(gru, f"weight_hh_l{k}").grad.numpy() for k in range(N)})
    tg.update(out_weight=lin.weight.grad.numpy(), out_bias=lin.bias.grad.numpy())
    t_out = rel_l2(tout.detach().numpy(), rout)
    t_err = _grad_errors(shape, tx.grad.numpy(), R.flat_weights(tg, I, H, N, O), *rfull)
    e_out = rel_l2(out, rout)
    e_err = _grad_errors(shape, dx, dw, *rfull)
    print(f"saturated: out ours {e_out:.2e} torch {t_out:.2e}; " +
          " ".join(f"{k} ours {e_err[k]:.2e} torch {t_err[k]:.2e}" for k in e_err))
    assert e_out <= 8 * t_out
    for k in e_err:
        assert e_err[k] <= 8 * t_err[k], (k, e_err[k], t_err[k])
