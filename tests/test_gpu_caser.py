"""The Caser convolution kernels on the GPU (bsarec_caser_fwd / bsarec_caser_bwd, csrc/caser.h) through ctypes against the fp64
restatement (caser_ref): every shape, padded ties, row independence, determinism, graph capture, train = 0, an undersized
workspace.  Inputs are caser_ref.random_case: x ~ N(0, 1) rounded to fp32, filters U(+-1/sqrt(fan_in)).  Gates: those of
test_gpu_gru.py (the fused-path gates of test_gpu_parity.py) -- z <= 2e-5 rel-L2 on every cell, every gradient tensor <= 2e-4 rel-L2.
The maximum is continuous, so nothing is masked in the forward.  The backward makes a discrete choice per cell (which window, and
whether ReLU passes): fp32 cannot be asked to reproduce one whose margin is at its rounding level, so dz is 0 on the cells that
caser_ref.ambiguous(cache, 1e-4) marks -- at most 0.2 % of a case's horizontal cells, a condition on the inputs that is asserted."""
import functools

import numpy as np
import pytest

from conftest import rel_l2
import caser_ref as R
from test_caser_cpu import padded_case

pytestmark = pytest.mark.gpu
OUT_GATE, GRAD_GATE, MARGIN, MASK_CAP = 2e-5, 2e-4, 1e-4, 0.002

SHAPES = [(1, 1, 4, 4, 1), (2, 2, 64, 16, 4), (3, 5, 8, 4, 2), (17, 12, 64, 16, 4), (33, 50, 64, 16, 4), (5, 20, 100, 8, 3),
          (2, 256, 16, 4, 1), (4, 50, 256, 32, 16)]
BIG = (33, 50, 64, 16, 4)


class Call:
    """Static buffers of one shape and the two entries on the current stream; outputs start as NaN."""

    def __init__(self, shape, x, flat, dz, train=1):
        import torch
        from bsarec_amd import _lib
        self.lib, self._lib = _lib.load(), _lib
        B, L, d, nh, nv = shape
        self.cfg = _lib.CaserConfig(B, L, d, nh, nv)
        self.nb = self.lib.bsarec_caser_workspace_bytes(self.cfg, train)
        assert self.nb > 0 and self.lib.bsarec_caser_weight_floats(self.cfg) == flat.size
        self.ws = torch.empty(self.nb, dtype=torch.uint8, device="cuda")
        self.x, self.flat = torch.from_numpy(np.ascontiguousarray(x)).cuda(), torch.from_numpy(flat).cuda()
        self.dz = None if dz is None else torch.from_numpy(np.ascontiguousarray(dz, dtype=np.float32)).cuda()
        self.z = torch.empty(B, nv * d + nh * L, device="cuda")
        self.dx, self.dw = torch.empty(B, L, d, device="cuda"), torch.empty(flat.size, device="cuda")
        self.train = int(train)
        self.poison()

    def poison(self):
        for t in (self.z, self.dx, self.dw):
            t.fill_(float("nan"))

    def launch(self):
        import torch
        st = torch.cuda.current_stream().cuda_stream
        self._lib.check(self.lib.bsarec_caser_fwd(self.cfg, self.x.data_ptr(), self.flat.data_ptr(), self.train, self.z.data_ptr(),
                                                  self.ws.data_ptr(), self.nb, st), "bsarec_caser_fwd")
        if self.dz is not None:
            self._lib.check(self.lib.bsarec_caser_bwd(self.cfg, self.x.data_ptr(), self.flat.data_ptr(), self.dz.data_ptr(),
                                                      self.ws.data_ptr(), self.nb, self.dx.data_ptr(), self.dw.data_ptr(), st),
                            "bsarec_caser_bwd")
        return self

    def results(self):
        return self.z.cpu().numpy(), self.dx.cpu().numpy(), self.dw.cpu().numpy()


def _reference(shape, x, flat, seed):
    """(dz fp32 with 0 on the ambiguous cells, z, dx, dflat, masked cells, cells) in fp64."""
    B, L, d, nh, nv = shape
    z, cache = R.forward(x, flat, nh, nv)
    dz = np.random.default_rng(seed).normal(0, 1, z.shape).astype(np.float32)
    amb = R.ambiguous(cache, MARGIN)
    dz[:, nv * d:][amb.reshape(B, L * nh)] = 0.0
    dx, dflat = R.backward(cache, dz)
    return dz, z, dx, dflat, int(amb.sum()), amb.size


@functools.lru_cache(maxsize=None)
def _case(shape):
    """fp32-rounded inputs and the fp64 reference, computed once per case."""
    x, flat = R.random_case(shape)
    return (x, flat) + _reference(shape, x, flat, sum(shape))


@functools.lru_cache(maxsize=None)
def _padded():
    ids, x, flat = padded_case()
    shape = (4, 12, 8, 4, 2)
    return (shape, x, flat) + _reference(shape, x, flat, 3)


def _grad_errors(shape, got_dx, got_dw, ref_dx, ref_dw):
    B, L, d, nh, nv = shape
    errs = {"dx": rel_l2(got_dx, ref_dx)}
    g, r = R.split_weights(got_dw, L, d, nh, nv), R.split_weights(ref_dw, L, d, nh, nv)
    worst = {}
    for k in r:
        kind = k if k.startswith("conv_v") else "conv_h.*." + k.rsplit(".", 1)[1]
        e = rel_l2(g[k], r[k]) if r[k].any() or g[k].any() else 0.0
        worst[kind] = max(worst.get(kind, 0.0), e)
        assert e <= GRAD_GATE, (k, e)                                    # every tensor, not the worst of a kind only
    errs.update(worst)
    return errs


def _gaps(shape, dw):
    B, L, d, nh, nv = shape
    lay, total = R.layout(L, d, nh, nv)
    covered = np.zeros(total, bool)
    for name, off, shp in lay:
        covered[off:off + int(np.prod(shp))] = True
    return dw[~covered]


@pytest.mark.parametrize("shape", SHAPES, ids=["-".join(map(str, s)) for s in SHAPES])
def test_kernel_vs_fp64_reference(shape):
    B, L, d, nh, nv = shape
    x, flat, dz, rz, rdx, rdw, masked, cells = _case(shape)
    print(f"caser {shape}: {masked} of {cells} horizontal cells masked ({100.0 * masked / cells:.3f} %)")
    assert masked <= MASK_CAP * cells                                     # a condition on the inputs
    z, dx, dw = Call(shape, x, flat, dz).launch().results()
    assert np.isfinite(z).all() and np.isfinite(dx).all() and np.isfinite(dw).all()      # every float overwritten
    e_z = rel_l2(z, rz)
    e_zh = rel_l2(z[:, nv * d:], rz[:, nv * d:])
    print(f"caser {shape}: z {e_z:.2e} zh {e_zh:.2e}")
    assert e_z <= OUT_GATE and e_zh <= OUT_GATE
    assert not _gaps(shape, dw).any()                                     # zeros in the gaps
    errs = _grad_errors(shape, dx, dw, rdx, rdw)
    print(f"caser {shape}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["dx"] <= GRAD_GATE


def test_padded_ties_follow_the_lowest_t():
    """Left-padded sequences and a constant row: windows repeat bit for bit, so ties among passing cells are exact.  The gradients
    follow the lowest t (the reference's rule), and identical windows give identical z bits."""
    shape, x, flat, dz, rz, rdx, rdw, masked, cells = _padded()
    B, L, d, nh, nv = shape
    assert masked <= MASK_CAP * cells
    z, dx, dw = Call(shape, x, flat, dz).launch().results()
    assert np.isfinite(z).all() and np.isfinite(dx).all() and np.isfinite(dw).all()
    assert rel_l2(z, rz) <= OUT_GATE
    errs = _grad_errors(shape, dx, dw, rdx, rdw)
    print("caser padded: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert errs["dx"] <= GRAD_GATE
    # identical windows give identical z bits, whatever their t.  Sequence 3 is one row repeated: each of its cells is the value of
    # its window 0.  A sequence that has that window elsewhere -- rows 0 .. 5 of sequence 2 followed by six copies of the row (the
    # window sits at t = 6 .. 12 - h for h <= 6), or the copies first (t = 0 .. 6 - h) -- and whose maximum the reference finds in it
    # must show the same bits in that cell.
    zh = z[:, nv * d:].reshape(B, L, nh)
    hits = 0
    for front in (False, True):
        x2 = x[2:3].copy()
        if front:
            x2[0, :6] = x[3, 0]
        else:
            x2[0, 6:] = x[3, 0]
        z2 = Call((1,) + shape[1:], x2, flat, None).launch().results()[0][:, nv * d:].reshape(L, nh)
        t2 = R.forward(x2, flat, nh, nv)[1][2][0]
        for h in range(1, 7):
            for f in range(nh):
                if t2[h - 1, f] == (0 if front else 6):                   # the lowest t of the repeated window attains the maximum
                    assert z2[h - 1, f].tobytes() == zh[3, h - 1, f].tobytes(), (front, h, f)
                    hits += 1
    assert hits >= 3                                                      # a condition on the inputs (3 with these)


def test_row_independence():
    """Sequence 7 of the (33, 50, 64, 16, 4) case, run alone as B = 1, gives the same z bits."""
    x, flat = _case(BIG)[:2]
    full = Call(BIG, x, flat, None).launch().results()[0]
    alone = Call((1,) + BIG[1:], np.ascontiguousarray(x[7:8]), flat, None).launch().results()[0]
    assert np.isfinite(full).all() and np.array_equal(full[7], alone[0])


@pytest.mark.parametrize("shape", [BIG, (5, 20, 100, 8, 3)], ids=["33-50-64-16-4", "5-20-100-8-3"])
def test_determinism_and_train0(shape):
    x, flat, dz = _case(shape)[:3]
    a = Call(shape, x, flat, dz).launch().results()
    b = Call(shape, x, flat, dz).launch().results()
    for u, v in zip(a, b):
        assert np.isfinite(u).all() and np.array_equal(u, v)
    c = Call(shape, x, flat, dz)
    c.launch()
    c.poison()
    again = c.launch().results()                      # the same workspace a second time
    for u, v in zip(a, again):
        assert np.array_equal(u, v)
    ev = Call(shape, x, flat, None, train=0).launch().results()[0]
    assert np.array_equal(ev, a[0])


def test_graph_capture():
    """Forward and backward captured once (one linear chain) and replayed three times give the bits of the eager call."""
    import torch
    x, flat, dz = _case(BIG)[:3]
    c = Call(BIG, x, flat, dz)
    eager = c.launch().results()                      # the warm-up: every kernel has run once before the capture
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


def test_undersized_workspace_is_refused():
    import torch
    shape = (3, 5, 8, 4, 2)
    x, flat, dz = _case(shape)[:3]
    c = Call(shape, x, flat, dz)
    st = torch.cuda.current_stream().cuda_stream
    assert c.lib.bsarec_caser_fwd(c.cfg, c.x.data_ptr(), c.flat.data_ptr(), 1, c.z.data_ptr(), c.ws.data_ptr(), c.nb - 1, st) < 0
    assert c.lib.bsarec_caser_bwd(c.cfg, c.x.data_ptr(), c.flat.data_ptr(), c.dz.data_ptr(), c.ws.data_ptr(), c.nb - 1,
                                  c.dx.data_ptr(), c.dw.data_ptr(), st) < 0
    small = c.lib.bsarec_caser_workspace_bytes(c.cfg, 0)
    assert small < c.nb
    assert c.lib.bsarec_caser_bwd(c.cfg, c.x.data_ptr(), c.flat.data_ptr(), c.dz.data_ptr(), c.ws.data_ptr(), small,
                                  c.dx.data_ptr(), c.dw.data_ptr(), st) < 0      # the backward needs the train = 1 size
    torch.cuda.synchronize()
    assert torch.isnan(c.z).all() and torch.isnan(c.dx).all()                    # nothing ran
