"""The selective state-space kernels on the GPU (bsarec_mamba_fwd / bsarec_mamba_bwd, csrc/mamba.h) through ctypes against the
fp64 restatement (mamba_ref): every shape under every padding pattern, every sequence length around the checkpoint distance,
the exact properties of padding, causality, row independence, determinism, train = 0 and graph capture.  Inputs are N(0, 1)
rounded to fp32, weights mamba_ref.random_weights (the model's init), dt_rank 4 ceil(d / 64).  Gates: the project's fp32 gates
of test_gpu_gru.py / test_gpu_lru.py -- out <= 2e-5 rel-L2, every gradient tensor <= 2e-4 rel-L2.

The training forward keeps the state after every CK-th step (CK = 8, MAMBA_CK of csrc/mamba.h) and the backward forms a
chunk's states again from its checkpoint, which is where ``CK_LENGTHS`` run."""
import functools

import numpy as np
import pytest

from conftest import rel_l2
import mamba_ref as R

pytestmark = pytest.mark.gpu
OUT_GATE, GRAD_GATE = 2e-5, 2e-4
CK = 8

# (B, L, d, E, N, K)
SHAPES = [(1, 1, 4, 1, 4, 2), (17, 2, 12, 2, 8, 4), (3, 3, 16, 2, 16, 4), (33, 15, 64, 2, 16, 4), (5, 17, 100, 2, 16, 3),
          (2, 256, 256, 2, 32, 4)]
CK_LENGTHS = [CK - 1, CK, CK + 1, 2 * CK, 2 * CK + 1]
SHAPES += [(2, L, 64, 2, 16, 4) for L in CK_LENGTHS]
MASKS = ["null", "ragged", "last", "checkpoint", "conv"]
_id = lambda s: "-".join(map(str, s))


def hyper_of(shape):
    B, L, d, E, N, K = shape
    return (E, N, K, R.dt_rank(d))


def make_ids(rng, shape, mask):
    """null: no ids; ragged: random first items, and row 0 padding alone when B > 1; last: the first item at L - 1;
    checkpoint: the first item on a checkpoint's first step, the rows cycling through the checkpoints (step 0 when L <= CK);
    conv: the first item at t with 0 < L - t < K, so the convolution window of every item straddles the boundary."""
    B, L, d, E, N, K = shape
    if mask == "null":
        return None
    if mask == "ragged":
        first = list(rng.integers(0, L, B))
        if B > 1:
            first[0] = L
    elif mask == "last":
        first = [L - 1] * B
    elif mask == "checkpoint":
        nck = -(-L // CK) - 1
        first = [CK * (1 + b % nck) if nck > 0 else 0 for b in range(B)]
    else:
        first = [max(0, L - 1 - b % (K - 1)) for b in range(B)]
    return R.ragged_ids(rng, B, L, first)


class Call:
    """Static buffers of one shape and the two entries on the current stream; workspace and outputs start as NaN."""

    def __init__(self, shape, x, ids, flat, dout, train=1):
        import torch
        from bsarec_amd import _lib
        self.lib, self._lib = _lib.load(), _lib
        B, L, d, E, N, K = shape
        self.cfg = _lib.MambaConfig(B, L, d, E, N, K, R.dt_rank(d))
        self.nb = self.lib.bsarec_mamba_workspace_bytes(self.cfg, train)
        assert self.nb > 0 and self.lib.bsarec_mamba_weight_floats(self.cfg) == flat.size
        self.ws = torch.empty(self.nb // 4, dtype=torch.float32, device="cuda")
        self.x, self.flat = torch.from_numpy(x).cuda(), torch.from_numpy(flat).cuda()
        self.ids = None if ids is None else torch.from_numpy(ids).cuda()
        self.dout = None if dout is None else torch.from_numpy(np.ascontiguousarray(dout, dtype=np.float32)).cuda()
        self.out, self.dx = torch.empty(B, L, d, device="cuda"), torch.empty(B, L, d, device="cuda")
        self.dw = torch.empty(flat.size, device="cuda")
        self.train = int(train)
        self.poison(True)

    def poison(self, workspace=False):
        for t in (self.out, self.dx, self.dw) + ((self.ws,) if workspace else ()):
            t.fill_(float("nan"))

    def launch(self, backward=True):
        import torch
        st = torch.cuda.current_stream().cuda_stream
        ids = None if self.ids is None else self.ids.data_ptr()
        self._lib.check(self.lib.bsarec_mamba_fwd(self.cfg, self.x.data_ptr(), ids, self.flat.data_ptr(), self.train,
                                                  self.out.data_ptr(), self.ws.data_ptr(), self.nb, st), "bsarec_mamba_fwd")
        if backward and self.dout is not None:
            self._lib.check(self.lib.bsarec_mamba_bwd(self.cfg, self.x.data_ptr(), ids, self.flat.data_ptr(), self.dout.data_ptr(),
                                                      self.ws.data_ptr(), self.nb, self.dx.data_ptr(), self.dw.data_ptr(), st),
                            "bsarec_mamba_bwd")
        return self

    def results(self):
        return self.out.cpu().numpy(), self.dx.cpu().numpy(), self.dw.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(shape, mask="ragged"):
    """fp32-rounded inputs and the fp64 reference, computed once per case and left alone."""
    B, L, d, E, N, K = shape
    rng = np.random.default_rng(7 * B + 11 * L + 13 * d + 17 * MASKS.index(mask) + N + K)
    x = rng.normal(0, 1, (B, L, d)).astype(np.float32)
    flat = R.random_weights(rng, d, *hyper_of(shape))
    dout = rng.normal(0, 1, (B, L, d)).astype(np.float32)
    ids = make_ids(rng, shape, mask)
    out, cache = R.forward(x, ids, flat, hyper_of(shape))
    return x, ids, flat, dout, out, R.backward(cache, dout)


def _errors(shape, got, ref):
    out, dx, dw = got
    rout, (rdx, rdw) = ref
    errs = {"out": rel_l2(out, rout), "dx": rel_l2(dx, rdx)}
    d = shape[2]
    g, r = R.split_weights(dw, d, *hyper_of(shape)), R.split_weights(rdw, d, *hyper_of(shape))
    for k in r:
        errs[k] = rel_l2(g[k], r[k])
    return errs


def _check(shape, mask):
    x, ids, flat, dout, rout, rgrad = _case(shape, mask)
    got = Call(shape, x, ids, flat, dout).launch().results()
    assert all(np.isfinite(t).all() for t in got)                     # every float overwritten
    errs = _errors(shape, got, (rout, rgrad))
    print(f"mamba parity {shape} {mask}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= (OUT_GATE if k == "out" else GRAD_GATE), (shape, mask, k, v)
    if ids is not None:                                               # padded positions: exact zeros
        pad = ids == 0
        assert not got[0][pad].view(np.uint32).any() and not got[1][pad].any()
    return got


@pytest.mark.parametrize("mask", MASKS)
@pytest.mark.parametrize("shape", SHAPES, ids=[_id(s) for s in SHAPES])
def test_kernel_vs_fp64_reference(shape, mask):
    _check(shape, mask)


def test_workload_shape_once():
    _check((256, 50, 64, 2, 16, 4), "ragged")


def test_null_ids_is_the_unmasked_layer():
    shape = (33, 15, 64, 2, 16, 4)
    x, _, flat, dout = _case(shape, "null")[:4]
    a = Call(shape, x, None, flat, dout).launch().results()
    b = Call(shape, x, np.ones(shape[:2], np.int64), flat, dout).launch().results()
    for u, v in zip(a, b):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))


_PAD_SHAPES = [(17, 2, 12, 2, 8, 4), (33, 15, 64, 2, 16, 4), (5, 17, 100, 2, 16, 3), (2, 33, 64, 2, 16, 4)]
_PAD_CASES = [(s, m) for m in ("ragged", "conv") for s in _PAD_SHAPES] + [(s, "checkpoint") for s in _PAD_SHAPES[2:]]


@pytest.mark.parametrize("shape,mask", _PAD_CASES, ids=[_id(s) + "-" + m for s, m in _PAD_CASES])
def test_padding_is_exact(shape, mask):
    """out = 0 bit for bit and dx = 0 at padded positions; other finite values of x under the padding change no bit of out or
    dx at an item's position and no bit of any weight gradient."""
    x, ids, flat, dout = _case(shape, mask)[:4]
    pad = ids == 0
    assert pad.any() and not pad.all()
    out, dx, dw = Call(shape, x, ids, flat, dout).launch().results()
    assert not out[pad].view(np.uint32).any() and not dx[pad].any()
    rng = np.random.default_rng(1)
    other = np.where(rng.random(x.shape) < 0.5, 3e6, -7.25).astype(np.float32)
    x2 = np.where(pad[..., None], other, x).astype(np.float32)
    out2, dx2, dw2 = Call(shape, x2, ids, flat, dout).launch().results()
    for u, v in ((out, out2), (dx, dx2), (dw, dw2)):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))


def test_all_padded_batch():
    for shape in ((1, 9, 64, 2, 16, 4), (6, 1, 12, 1, 4, 2)):
        rng = np.random.default_rng(shape[1])
        x, dout = rng.normal(0, 1, shape[:3]).astype(np.float32), rng.normal(0, 1, shape[:3]).astype(np.float32)
        flat = R.random_weights(rng, shape[2], *hyper_of(shape))
        out, dx, dw = Call(shape, x, np.zeros(shape[:2], np.int64), flat, dout).launch().results()
        assert not out.any() and not dx.any() and not dw.any()


def test_causality():
    """Changing x behind position s changes no bit of out[:, :s + 1]."""
    shape = (5, 17, 100, 2, 16, 3)
    x, ids, flat, dout = _case(shape, "ragged")[:4]
    out = Call(shape, x, ids, flat, None).launch().results()[0]
    for s in (0, 7, 15):
        x2 = x.copy()
        x2[:, s + 1:] += 1.5
        out2 = Call(shape, x2, ids, flat, None).launch().results()[0]
        assert np.array_equal(out2[:, :s + 1].view(np.uint32), out[:, :s + 1].view(np.uint32))
        assert not np.array_equal(out2[:, s + 1:], out[:, s + 1:])


@pytest.mark.parametrize("shape", [(33, 15, 64, 2, 16, 4), (33, 20, 12, 2, 8, 3)], ids=_id)
def test_row_independence(shape):
    """A sequence run alone as B = 1 has the bits it has at two places of a batch of 33, forward and dx."""
    B, L = shape[:2]
    x, ids, flat, dout = _case(shape, "ragged")[:4]
    b = next(i for i in range(1, B) if ids[i, L // 2] != 0 and ids[i, 0] == 0)
    alone = Call((1,) + shape[1:], np.ascontiguousarray(x[b:b + 1]), np.ascontiguousarray(ids[b:b + 1]), flat,
                 dout[b:b + 1]).launch().results()
    for place in (2, 32):
        x2, ids2, dout2 = x.copy(), ids.copy(), dout.copy()
        x2[place], ids2[place], dout2[place] = x[b], ids[b], dout[b]
        out, dx, _ = Call(shape, x2, ids2, flat, dout2).launch().results()
        assert np.array_equal(out[place].view(np.uint32), alone[0][0].view(np.uint32))
        assert np.array_equal(dx[place].view(np.uint32), alone[1][0].view(np.uint32))


@pytest.mark.parametrize("shape", [(33, 15, 64, 2, 16, 4), (5, 17, 100, 2, 16, 3), (2, 33, 64, 2, 16, 4)], ids=_id)
def test_determinism_and_train0(shape):
    x, ids, flat, dout = _case(shape, "ragged")[:4]
    a = Call(shape, x, ids, flat, dout).launch().results()
    b = Call(shape, x, ids, flat, dout).launch().results()
    for u, v in zip(a, b):
        assert np.isfinite(u).all() and np.array_equal(u.view(np.uint32), v.view(np.uint32))
    c = Call(shape, x, ids, flat, dout)
    c.launch()
    c.poison()
    again = c.launch().results()                      # the same workspace a second time
    for u, v in zip(a, again):
        assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
    ev = Call(shape, x, ids, flat, None, train=0).launch().results()[0]
    assert np.array_equal(ev.view(np.uint32), a[0].view(np.uint32))


def test_graph_capture():
    """Forward and backward captured once and replayed twice give the bits of the eager call."""
    import torch
    shape = (2, 33, 64, 2, 16, 4)
    x, ids, flat, dout = _case(shape, "ragged")[:4]
    c = Call(shape, x, ids, flat, dout)
    eager = c.launch().results()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c.launch()
    for _ in range(2):
        c.poison(True)
        graph.replay()
        torch.cuda.synchronize()
        for u, v in zip(eager, c.results()):
            assert np.array_equal(u.view(np.uint32), v.view(np.uint32))
