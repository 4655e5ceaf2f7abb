"""The linear recurrent unit kernels on the GPU (bsarec_lru_fwd / bsarec_lru_bwd, csrc/lru.h) through ctypes against the fp64
restatement (lru_ref): every shape under every padding pattern, every sequence length at which the scan's chunk length changes,
the exact properties of padding and of L = 1, row independence, determinism, train = 0, graph capture, long and short memory.
Inputs are N(0, 1) rounded to fp32, weights lru_ref.random_weights (the ring init of the model).  Gates: the project's fp32
gates of test_gpu_gru.py / test_gpu_parity.py -- y <= 2e-5 rel-L2, every gradient tensor <= 2e-4 rel-L2.

The scan splits time into NC = min(16, 256 // (d // 4)) chunks of CL = ceil(L / NC) steps (csrc/lru.h): CL changes between
L = k NC and k NC + 1, which is where ``test_every_chunk_edge`` runs."""
import functools

import numpy as np
import pytest

from conftest import rel_l2
import lru_ref as R

pytestmark = pytest.mark.gpu
OUT_GATE, GRAD_GATE = 2e-5, 2e-4

SHAPES = [(1, 1, 4), (17, 2, 12), (33, 15, 64), (16, 16, 64), (5, 17, 100), (256, 50, 64), (3, 255, 256), (2, 256, 256)]
MASKS = ["none", "ragged", "last", "edge"]


def chunking(L, d):
    nc = min(16, 256 // (d // 4))
    cl = -(-L // nc)
    return nc, cl, -(-L // cl)


def make_ids(rng, shape, mask):
    """none: no padding; ragged: random first items, and row 0 padding alone when B > 1; last: the first item at L - 1;
    edge: the first item exactly on a chunk's first step, the rows cycling through the chunks."""
    B, L, d = shape
    nc, cl, nu = chunking(L, d)
    if mask == "none":
        first = [0] * B
    elif mask == "ragged":
        first = list(rng.integers(0, L, B))
        if B > 1:
            first[0] = L
    elif mask == "last":
        first = [L - 1] * B
    else:
        first = [cl * (1 + b % (nu - 1)) if nu > 1 else 0 for b in range(B)]
    return R.ragged_ids(rng, B, L, first)


class Call:
    """Static buffers of one shape and the two entries on the current stream; workspace and outputs start as NaN."""

    def __init__(self, shape, x, ids, flat, dy, train=1):
        import torch
        from bsarec_amd import _lib
        self.lib, self._lib = _lib.load(), _lib
        B, L, d = shape
        self.cfg = _lib.LruConfig(B, L, d)
        self.nb = self.lib.bsarec_lru_workspace_bytes(self.cfg, train)
        assert self.nb > 0 and self.lib.bsarec_lru_weight_floats(self.cfg) == flat.size
        self.ws = torch.empty(self.nb // 4, dtype=torch.float32, device="cuda")
        self.x, self.flat = torch.from_numpy(x).cuda(), torch.from_numpy(flat).cuda()
        self.ids = None if ids is None else torch.from_numpy(ids).cuda()
        self.dy = None if dy is None else torch.from_numpy(np.ascontiguousarray(dy, dtype=np.float32)).cuda()
        self.y, self.dx = torch.empty(B, L, d, device="cuda"), torch.empty(B, L, d, device="cuda")
        self.dw = torch.empty(flat.size, device="cuda")
        self.train = int(train)
        self.poison(True)

    def poison(self, workspace=False):
        for t in (self.y, self.dx, self.dw) + ((self.ws,) if workspace else ()):
            t.fill_(float("nan"))

    def launch(self, backward=True):
        import torch
        st = torch.cuda.current_stream().cuda_stream
        ids = None if self.ids is None else self.ids.data_ptr()
        self._lib.check(self.lib.bsarec_lru_fwd(self.cfg, self.x.data_ptr(), ids, self.flat.data_ptr(), self.train, self.y.data_ptr(),
                                                self.ws.data_ptr(), self.nb, st), "bsarec_lru_fwd")
        if backward and self.dy is not None:
            self._lib.check(self.lib.bsarec_lru_bwd(self.cfg, self.x.data_ptr(), ids, self.flat.data_ptr(), self.dy.data_ptr(),
                                                    self.ws.data_ptr(), self.nb, self.dx.data_ptr(), self.dw.data_ptr(), st),
                            "bsarec_lru_bwd")
        return self

    def results(self):
        return self.y.cpu().numpy(), self.dx.cpu().numpy(), self.dw.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(shape, mask="ragged", nu_log=None):
    """fp32-rounded inputs and the fp64 reference, computed once per case and left alone."""
    B, L, d = shape
    rng = np.random.default_rng(7 * B + 11 * L + 13 * d + 17 * MASKS.index(mask if mask in MASKS else "none"))
    x = rng.normal(0, 1, (B, L, d)).astype(np.float32)
    flat = R.random_weights(rng, d, nu_log=nu_log)
    dy = rng.normal(0, 1, (B, L, d)).astype(np.float32)
    ids = None if mask == "null" else make_ids(rng, shape, mask)
    y, cache = R.forward(x, ids, flat)
    return x, ids, flat, dy, y, R.backward(cache, dy)


def _errors(d, got, ref):
    y, dx, dw = got
    ry, (rdx, rdw) = ref
    errs = {"y": rel_l2(y, ry), "dx": rel_l2(dx, rdx)}
    g, r = R.split_weights(dw, d), R.split_weights(rdw, d)
    for k in r:
        errs[k] = rel_l2(g[k], r[k])
    return errs


def _check(shape, mask, label):
    x, ids, flat, dy, ry, rgrad = _case(shape, mask)
    got = Call(shape, x, ids, flat, dy).launch().results()
    assert all(np.isfinite(t).all() for t in got)                     # every float overwritten
    errs = _errors(shape[2], got, (ry, rgrad))
    print(f"lru {label} {shape} {mask}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= (OUT_GATE if k == "y" else GRAD_GATE), (shape, mask, k, v)
    if shape[1] == 1:
        g = R.split_weights(got[2], shape[2])
        assert not g["nu_log"].any() and not g["theta_log"].any()     # no t >= 1: exactly zero
    return got


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=["-".join(map(str, s)) for s in SHAPES])
def test_kernel_vs_fp64_reference(shape, mask):
    _check(shape, mask, "parity")


def test_null_ids_is_the_unmasked_layer():
    shape = (33, 15, 64)
    _check(shape, "null", "null ids")
    x, _, flat, dy = _case(shape, "null")[:4]
    a = Call(shape, x, None, flat, dy).launch().results()
    b = Call(shape, x, np.ones(shape[:2], np.int64), flat, dy).launch().results()
    for u, v in zip(a, b):
        assert np.array_equal(u, v)


@pytest.mark.parametrize("d", [64, 256])
def test_every_chunk_edge(d):
    """L = k NC and k NC + 1 for every k: the chunk length steps from k to k + 1 between them (d = 64: NC = 16; d = 256: NC = 4).
    Ragged rows, so the first items fall inside chunks as well."""
    nc = chunking(256, d)[0]
    worst = {}
    for k in range(1, 256 // nc):
        for L in (k * nc, k * nc + 1):
            shape = (2, L, d)
            x, ids, flat, dy, ry, rgrad = _case(shape, "ragged")
            got = Call(shape, x, ids, flat, dy).launch().results()
            assert all(np.isfinite(t).all() for t in got)
            for name, v in _errors(d, got, (ry, rgrad)).items():
                assert v <= (OUT_GATE if name == "y" else GRAD_GATE), (shape, name, v)
                worst[name] = max(worst.get(name, 0.0), v)
    print(f"lru chunk edges d={d}: worst " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))


@pytest.mark.parametrize("shape", [(17, 2, 12), (33, 15, 64), (5, 17, 100), (3, 255, 256)], ids=lambda s: "-".join(map(str, s)))
def test_padding_is_exact(shape):
    """A row of padding alone: y = out_proj.bias bit for bit and dx = 0.  Large values of x under the padding change no bit
    of y at an item's position."""
    B, L, d = shape
    x, ids, flat, dy = _case(shape, "ragged")[:4]
    assert not ids[0].any()
    y, dx, dw = Call(shape, x, ids, flat, dy).launch().results()
    bias = R.split_weights(flat, d)["out_proj.bias"]
    assert np.array_equal(y[0].view(np.uint32), np.ascontiguousarray(np.broadcast_to(bias, (L, d))).view(np.uint32))
    assert not dx[0].any() and not dx[ids == 0].any()
    x2 = np.where((ids == 0)[..., None], np.float32(3e6), x).astype(np.float32)
    y2 = Call(shape, x2, ids, flat, None).launch().results()[0]
    real = ids != 0
    assert real.any() and np.array_equal(y2[real].view(np.uint32), y[real].view(np.uint32))


def test_all_padded_single_row_and_length_one():
    for shape in ((1, 9, 64), (1, 1, 4), (6, 1, 12)):
        B, L, d = shape
        rng = np.random.default_rng(L + d)
        x, dy = rng.normal(0, 1, shape).astype(np.float32), rng.normal(0, 1, shape).astype(np.float32)
        flat = R.random_weights(rng, d)
        ids = np.zeros((B, L), np.int64)
        y, dx, dw = Call(shape, x, ids, flat, dy).launch().results()
        w, g = R.split_weights(flat, d), R.split_weights(dw, d)
        assert np.array_equal(y, np.broadcast_to(w["out_proj.bias"], shape)) and not dx.any()
        for k in ("nu_log", "theta_log", "gamma_log", "in_proj.weight", "in_proj.bias", "out_proj.weight"):
            assert not g[k].any(), k
        assert rel_l2(g["out_proj.bias"], dy.astype(np.float64).sum((0, 1))) <= GRAD_GATE
        if L == 1:                                                    # with items too: dnu_log = dtheta_log = 0 exactly
            g = R.split_weights(Call(shape, x, None, flat, dy).launch().results()[2], d)
            assert not g["nu_log"].any() and not g["theta_log"].any() and g["gamma_log"].any()


@pytest.mark.parametrize("shape", [(33, 50, 64), (33, 15, 12)], ids=["33-50-64", "33-15-12"])
def test_row_independence(shape):
    """A sequence run alone as B = 1 has the bits it has at two places of a batch of 33, forward and dx (d = 12: five
    sequences share a workgroup; d = 64: one)."""
    B, L, d = shape
    x, ids, flat, dy = _case(shape, "ragged")[:4]
    b = 7
    assert ids[b].any()
    alone = Call((1, L, d), np.ascontiguousarray(x[b:b + 1]), np.ascontiguousarray(ids[b:b + 1]), flat, dy[b:b + 1]).launch().results()
    for place in (2, 32):
        x2, ids2, dy2 = x.copy(), ids.copy(), dy.copy()
        x2[place], ids2[place], dy2[place] = x[b], ids[b], dy[b]
        y, dx, _ = Call(shape, x2, ids2, flat, dy2).launch().results()
        assert np.array_equal(y[place].view(np.uint32), alone[0][0].view(np.uint32))
        assert np.array_equal(dx[place].view(np.uint32), alone[1][0].view(np.uint32))


@pytest.mark.parametrize("shape", [(33, 50, 64), (5, 17, 100)], ids=["33-50-64", "5-17-100"])
def test_determinism_and_train0(shape):
    x, ids, flat, dy = _case(shape, "ragged")[:4]
    a = Call(shape, x, ids, flat, dy).launch().results()
    b = Call(shape, x, ids, flat, dy).launch().results()
    for u, v in zip(a, b):
        assert np.isfinite(u).all() and np.array_equal(u.view(np.uint32), v.view(np.uint32))
    c = Call(shape, x, ids, flat, dy)
    c.launch()
    c.poison()
    again = c.launch().results()                      # the same workspace a second time
    for u, v in zip(a, again):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
    ev = Call(shape, x, ids, flat, None, train=0).launch().results()[0]
    assert np.array_equal(ev.view(np.uint32), a[0].view(np.uint32))


def test_graph_capture():
    """Forward and backward captured once and replayed three times give the bits of the eager call."""
    import torch
    shape = (33, 50, 64)
    x, ids, flat, dy = _case(shape, "ragged")[:4]
    c = Call(shape, x, ids, flat, dy)
    eager = c.launch().results()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c.launch()
    for _ in range(3):
        c.poison(True)
        graph.replay()
        torch.cuda.synchronize()
        for u, v in zip(eager, c.results()):
            assert np.array_equal(u.view(np.uint32), v.view(np.uint32))


@pytest.mark.parametrize("nu_log", [-7.0, 2.0], ids=["long", "short"])
def test_long_and_short_memory(nu_log):
    """nu_log ~ -7 (|lambda| ~ 0.999: 256 steps are all remembered) and ~ +2 (|lambda| ~ 6e-4: one step).  The fixed gates do
    not apply -- the plain fp32 numpy restatement of the same inputs is itself at y 2.4e-5 and dtheta_log 2.3e-4 in the long
    case -- so every tensor is gated at 8 x the error of that restatement against fp64, computed here (test_gpu_gru.py's
    test_saturated_gates is the precedent)."""
    shape = (5, 256, 64)
    x, ids, flat, dy, ry, rgrad = _case(shape, "ragged", nu_log)
    got = Call(shape, x, ids, flat, dy).launch().results()
    assert all(np.isfinite(t).all() for t in got)
    y32, c32 = R.forward(x, ids, flat, np.float32)
    ref32 = (y32,) + R.backward(c32, dy)
    assert all(t.dtype == np.float32 for t in ref32)
    ours, plain = _errors(64, got, (ry, rgrad)), _errors(64, ref32, (ry, rgrad))
    print(f"lru nu_log={nu_log}: " + " ".join(f"{k} ours {ours[k]:.2e} fp32 {plain[k]:.2e}" for k in ours))
    for k in ours:
        assert ours[k] <= 8 * plain[k], (k, ours[k], plain[k])
