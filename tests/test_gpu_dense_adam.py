"""The dense Adam family (``adam_kernel`` behind bsarec_adam_step / bsarec_adam_apply, and the two arms of ``reduce_adam_kernel``
behind bsarec_train_step_indexed; csrc/kernels.h) against the numpy restatement of tests/lazy_adam_ref.py and a float64 Adam.

Plan-less: synthetic arenas and a zeroed 64-byte state; every step the reference is fed the kernel's own previous w, m, v, so the
gate is that of one step: rel-L2 <= 1e-6 on w, m and v (the gate of test_gpu_lazy_adam._steps_against_restatement).  Covered: the
float4 tail and the grid-stride loop (n above 2048 x 256 groups), weight decay, non-default betas and eps, ``grad_scale``,
``grads2`` on a prefix, 1 / 2 / 8 gradient sources summed in index order, the bf16 shadow, the bias corrections up to t = 1,000,
the restart at t = 0, bsarec_adam_apply, the refusals.
Model level: three steps of bsarec_train_step and of bsarec_train_step_indexed with weight decay, betas (0.8, 0.95) and eps 1e-3,
every tensor's w, m, v against the restatement, the two entry points bit for bit against each other, fp32 and bf16 storage."""
import argparse
import ctypes as C

import numpy as np
import pytest

import lazy_adam_ref as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LR = 1e-3
N_TAIL, N_STRIDE = 4 * 257, 4 * (2048 * 256 + 257)      # one block + one group; past the 2048-block grid: the grid-stride loop
HYPER = [(wd, betas, eps, gs) for wd in (0.0, 0.01) for betas in ((0.9, 0.999), (0.8, 0.95)) for eps in (1e-8, 1e-3)
         for gs in (1.0, 0.5)]


def _values(rng, n):
    """Mixed signs, magnitudes 1e-8 .. 10, some exact zeros."""
    x = (rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-8, 1, size=n)).astype(np.float32)
    x[rng.random(n) < 0.05] = 0.0
    return x


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


class _Arena:
    """w, m, v, grads on the device, a zeroed step state, and the bsarec_adam_t that points at them."""

    def __init__(self, n, rng, wd=0.0, betas=(0.9, 0.999), eps=1e-8, gs=1.0, alloc=None):
        from bsarec_amd import _lib as Lb
        self.lib = Lb.load()
        self.n, self.hyper = n, (LR, betas[0], betas[1], eps)
        self.wd, self.gs = wd, gs
        alloc = alloc or n
        self.w = _dev((rng.standard_normal(alloc) * 0.1).astype(np.float32))
        self.g = _dev(_values(rng, alloc))
        self.m, self.v = torch.zeros_like(self.w), torch.zeros_like(self.w)
        self.state = torch.zeros(8, dtype=torch.int64, device="cuda")
        self.ad = Lb.Adam(self.w.data_ptr(), self.g.data_ptr(), self.m.data_ptr(), self.v.data_ptr(), n, LR, betas[0], betas[1],
                          eps, wd, gs, None, 0)

    def call(self, fn="bsarec_adam_step"):
        rc = getattr(self.lib, fn)(C.byref(self.ad), self.state.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        return rc

    def host(self):
        return tuple(x.cpu().numpy() for x in (self.w, self.m, self.v))

    def corrections(self):
        return self.state[3:4].view(torch.float32).cpu().numpy().copy()

    def check(self, before, g, t, what=""):
        """w, m, v now against one step t of the restatement (and of the float64 Adam) from ``before`` with gradient ``g``
        (dense_grad's: scale and weight decay already applied)."""
        lr, b1, b2, eps = self.hyper
        n = self.n
        want = R.dense_step(before[0][:n], before[1][:n], before[2][:n], g, t, lr, b1, b2, eps, 0.0)
        want64 = R.adam_f64(before[0][:n], before[1][:n], before[2][:n], g, t, lr, b1, b2, eps)
        for name, got, a, b in zip("wmv", self.host(), want, want64):
            assert np.isfinite(got).all()
            assert rel_l2(got[:n], a) <= 1e-6, (what, t, name, rel_l2(got[:n], a))
            assert rel_l2(got[:n], b) <= 1e-6, (what, t, name, "float64", rel_l2(got[:n], b))
            assert np.array_equal(got[n:], before["wmv".index(name)][n:]), (what, name, "written past n")


@pytest.mark.parametrize("wd,betas,eps,gs", HYPER)
@pytest.mark.parametrize("n", [4, N_TAIL, N_STRIDE])
def test_five_steps_vs_restatement(n, wd, betas, eps, gs):
    rng = np.random.default_rng(n + int(1000 * wd) + int(10 * betas[0]))
    A = _Arena(n, rng, wd, betas, eps, gs, alloc=n + 8)          # 8 floats past n: nothing may be written there
    for t in range(1, 6):
        A.g.copy_(_dev(_values(rng, n + 8)))
        before, g = A.host(), A.g.cpu().numpy()
        assert A.call() == 0
        A.check(before, R.dense_grad(g[:n], before[0][:n], gs, wd), t)
        assert int(A.state[2].item()) == t
        assert not np.array_equal(A.host()[0][:n], before[0][:n])


def test_weight_decay_moves_the_update():
    """The same step with and without weight decay differs by far more than the gate: the wd term is not lost in the tolerance."""
    rng = np.random.default_rng(0)
    g = _values(rng, N_TAIL)
    w = (rng.standard_normal(N_TAIL) * 0.1).astype(np.float32)
    z = np.zeros_like(w)
    a = R.dense_step(w, z, z, R.dense_grad(g, w, 1.0, 0.01), 1, LR, 0.9, 0.999, 1e-8, 0.0)
    b = R.dense_step(w, z, z, R.dense_grad(g, w, 1.0, 0.0), 1, LR, 0.9, 0.999, 1e-8, 0.0)
    assert rel_l2(a[1], b[1]) > 1e-4 and rel_l2(a[2], b[2]) > 1e-4


def test_grads2_is_added_on_its_prefix_and_zeroed_there():
    rng = np.random.default_rng(1)
    n, n2 = N_TAIL, 4 * 100
    A = _Arena(n, rng, wd=0.01, gs=0.5)
    g2 = _dev(_values(rng, n))
    A.ad.grads2, A.ad.grads2_n = g2.data_ptr(), n2
    for t in range(1, 3):
        g2.copy_(_dev(_values(rng, n)))
        before, g, g2_0 = A.host(), A.g.cpu().numpy(), g2.cpu().numpy()
        assert A.call() == 0
        want = R.dense_grad(g, before[0], 0.5, 0.01, grads2=g2_0, grads2_n=n2)
        assert not np.array_equal(want[:n2], R.dense_grad(g, before[0], 0.5, 0.01)[:n2])
        A.check(before, want, t)
        got2 = g2.cpu().numpy()
        assert not got2[:n2].any()
        assert np.array_equal(got2[n2:].view(np.uint32), g2_0[n2:].view(np.uint32))
        assert np.array_equal(A.g.cpu().numpy().view(np.uint32), g.view(np.uint32))


@pytest.mark.parametrize("nsrc", [1, 2, 8])
def test_gradient_sources_are_summed_in_index_order(nsrc):
    rng = np.random.default_rng(10 + nsrc)
    n = N_TAIL
    srcs = [_values(rng, n) for _ in range(nsrc)]
    dsrc = [_dev(s) for s in srcs]
    want = R.dense_grad(None, None, srcs=srcs)
    if nsrc == 8:                        # the order is observable: the reversed float32 sum differs somewhere
        assert not np.array_equal(want, R.dense_grad(None, None, srcs=srcs[::-1]))
    # beta1 = 0, no weight decay, scale 1: m = 0 * m + (1 - 0) * g is g itself, so the kernel's sum can be read bit for bit
    A = _Arena(n, rng, betas=(0.0, 0.999))
    A.g.fill_(float("nan"))              # `grads` is ignored
    A.ad.n_grad_srcs = nsrc
    for r, s in enumerate(dsrc):
        A.ad.grad_srcs[r] = s.data_ptr()
    before = A.host()
    assert A.call() == 0
    assert np.array_equal(A.host()[1], want)
    A.check(before, want, 1)
    # and through the ordinary hyper-parameters, scaled and decayed
    B = _Arena(n, rng, wd=0.01, betas=(0.8, 0.95), eps=1e-3, gs=0.5)
    B.g.fill_(float("nan"))
    B.ad.n_grad_srcs = nsrc
    for r, s in enumerate(dsrc):
        B.ad.grad_srcs[r] = s.data_ptr()
    for t in range(1, 3):
        before = B.host()
        assert B.call() == 0
        B.check(before, R.dense_grad(None, before[0], 0.5, 0.01, srcs=srcs), t)
    for s, d in zip(srcs, dsrc):
        assert np.array_equal(d.cpu().numpy().view(np.uint32), s.view(np.uint32))


def test_bf16_shadow_is_written_from_shadow_from_on():
    rng = np.random.default_rng(2)
    n, lo = N_TAIL, 4 * 64
    A = _Arena(n, rng, wd=0.01)
    shadow = torch.full((n,), 3.0, dtype=torch.bfloat16, device="cuda")
    A.ad.shadow_bf16, A.ad.shadow_from = shadow.data_ptr(), lo
    before, g = A.host(), A.g.cpu().numpy()
    assert A.call() == 0
    A.check(before, R.dense_grad(g, before[0], 1.0, 0.01), 1)
    assert torch.equal(shadow[lo:].view(torch.int16), A.w[lo:].to(torch.bfloat16).view(torch.int16))
    assert not torch.equal(shadow[lo:], torch.full_like(shadow[lo:], 3.0))
    assert torch.equal(shadow[:lo], torch.full_like(shadow[:lo], 3.0))


def _ulp_close(got, want):
    want = np.float32(want)
    return abs(float(np.float32(got)) - float(want)) <= float(np.spacing(np.abs(want)))


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.8, 0.95)])
def test_bias_corrections_over_a_thousand_steps(betas):
    """state[3] = {lr / (1 - b1^t), sqrt(1 - b2^t)}: the kernel keeps b^t as a float64 running product (within about 1e-13 of
    pow after 1,000 factors), so both floats are within 1 ulp of the float64 formula evaluated with pow."""
    rng = np.random.default_rng(3)
    A = _Arena(8, rng, betas=betas)
    lr, b1, b2 = (float(np.float32(x)) for x in (LR, betas[0], betas[1]))
    seen = []
    for t in range(1, 1001):
        rc = A.lib.bsarec_adam_step(C.byref(A.ad), A.state.data_ptr(), torch.cuda.current_stream().cuda_stream)
        assert rc == 0
        if t in (1, 2, 10, 100, 1000):
            torch.cuda.synchronize()
            f = A.corrections()
            assert int(A.state[2].item()) == t
            assert _ulp_close(f[0], lr / (1.0 - b1 ** t)), (t, f[0], lr / (1.0 - b1 ** t))
            assert _ulp_close(f[1], np.sqrt(1.0 - b2 ** t)), (t, f[1], np.sqrt(1.0 - b2 ** t))
            ss, bc = R.corrections(t, LR, betas[0], betas[1])
            assert _ulp_close(f[0], ss) and _ulp_close(f[1], bc)
            seen.append(t)
    assert seen == [1, 2, 10, 100, 1000]
    assert np.isfinite(A.host()[0]).all()


def test_t_zero_restarts_adam_and_apply_reuses_the_corrections():
    rng = np.random.default_rng(4)
    n = N_TAIL
    A = _Arena(n, rng, wd=0.01, betas=(0.8, 0.95), eps=1e-3)
    for t in range(1, 4):
        assert A.call() == 0
    f3 = A.corrections()
    # bsarec_adam_apply: the update alone -- same t, same corrections, a new gradient
    A.g.copy_(_dev(_values(rng, n)))
    before, g, st = A.host(), A.g.cpu().numpy(), A.state.clone()
    assert A.call("bsarec_adam_apply") == 0
    assert torch.equal(A.state, st)
    A.check(before, R.dense_grad(g, before[0], 1.0, 0.01), 3, "apply")
    # t = 0 restarts: the next step's corrections are those of t = 1, the moments stay
    A.state[2] = 0
    before = A.host()
    assert A.call() == 0
    f1 = A.corrections()
    assert int(A.state[2].item()) == 1
    ss, bc = R.corrections(1, LR, 0.8, 0.95)
    assert _ulp_close(f1[0], ss) and _ulp_close(f1[1], bc) and not _ulp_close(f1[0], f3[0]) and not _ulp_close(f1[1], f3[1])
    A.check(before, R.dense_grad(g, before[0], 1.0, 0.01), 1, "restart")


def test_refusals_change_nothing():
    rng = np.random.default_rng(5)
    n = N_TAIL
    A = _Arena(n, rng)
    assert A.call() == 0
    other = _dev(_values(rng, n))
    keep = [x.clone() for x in (A.w, A.m, A.v, A.g, A.state, other)]

    def refused(**fields):
        saved = {k: getattr(A.ad, k) for k in fields}
        for k, v in fields.items():
            setattr(A.ad, k, v)
        try:
            for fn in ("bsarec_adam_step", "bsarec_adam_apply"):
                assert A.call(fn) < 0, (fields, fn)
        finally:
            for k, v in saved.items():
                setattr(A.ad, k, v)
        for now, was in zip((A.w, A.m, A.v, A.g, A.state, other), keep):
            assert torch.equal(now, was), fields

    refused(n=n - 2)
    refused(grads2=other.data_ptr(), grads2_n=n + 4)
    refused(n_grad_srcs=9)
    A.ad.grad_srcs[0] = other.data_ptr()
    refused(n_grad_srcs=2)               # grad_srcs[1] is null
    A.ad.grad_srcs[0] = None
    assert A.call() == 0                 # the struct is whole again
    assert int(A.state[2].item()) == 2


# ---- model level: the separate adam_kernel (train_step) and the fused reduce_adam_kernel (train_step_indexed) ---------------------

WD, BETAS, EPS = 0.01, (0.8, 0.95), 1e-3


def _model(storage, state_dict=None):
    from bsarec_amd import BSARecModel
    a = argparse.Namespace(item_size=301, hidden_size=64, max_seq_length=50, batch_size=64, hidden_dropout_prob=0.3,
                           attention_probs_dropout_prob=0.2, num_hidden_layers=2, num_attention_heads=2, hidden_act="gelu",
                           initializer_range=0.02, c=3, alpha=0.9, seed=42, storage=storage)
    torch.manual_seed(0)
    m = BSARecModel(a)
    if state_dict is not None:
        m.load_state_dict(state_dict)
    m = m.cuda()
    m.configure_adam(lr=LR, betas=BETAS, eps=EPS, weight_decay=WD)
    m.set_seed(77)
    m.train()
    return m


@pytest.mark.parametrize("storage", [None, "bf16"])
def test_model_steps_both_entry_points_vs_restatement(storage):
    V, B, L = 301, 64, 50
    eager = _model(storage)
    indexed = _model(storage, eager.state_dict())
    assert torch.equal(eager._arena, indexed._arena)
    rng = np.random.default_rng(6)
    for t in range(1, 4):
        ids = rng.integers(1, V, size=(B, L)).astype(np.int64)
        ids[rng.random((B, L)) < 0.3] = 0
        ans = rng.integers(1, V, size=B).astype(np.int64)
        for m in (eager, indexed):
            before = tuple(x.cpu().numpy() for x in (m._arena, m._adam["m"], m._adam["v"]))
            if m is eager:
                m.train_step(_dev(ids), _dev(ans))
            else:
                if t == 1:
                    # train_step advances the dropout counter before it uses it, the indexed step uses it as it stands and advances
                    # it when the step closes (BSARecModel._fresh_step_counter): flag one begin-style step, so that the first
                    # indexed step begins the counter once and both models draw the masks of steps 1, 2, 3
                    m._step_begun = True
                m.train_step_indexed(_dev(ids), _dev(ans), torch.arange(B, dtype=torch.int64, device="cuda"),
                                     torch.zeros(1, dtype=torch.int64, device="cuda"), B)
            torch.cuda.synchronize()
            assert int(m._state[2].item()) == t and int(m._state[1].item()) == (t if m is eager else t + 1)
            g = m._garena.cpu().numpy()
            want = R.dense_step(*before, R.dense_grad(g, before[0], 1.0, WD), t, LR, BETAS[0], BETAS[1], EPS, 0.0)
            now = tuple(x.cpu().numpy() for x in (m._arena, m._adam["m"], m._adam["v"]))
            for k, (o, n, _) in m._slices.items():
                assert k.endswith("key.bias") or np.any(g[o:o + n]), k
                for name, got, ref in zip("wmv", now, want):
                    assert rel_l2(got[o:o + n], ref[o:o + n]) <= 1e-6, (t, k, name, rel_l2(got[o:o + n], ref[o:o + n]))
            if storage == "bf16":
                assert m._plan(B).bf16
                lo = m._slices["position_embeddings.weight"][0]
                assert torch.equal(m._shadow[lo:].view(torch.int16), m._arena[lo:].to(torch.bfloat16).view(torch.int16))
        for name, a, b in (("w", eager._arena, indexed._arena), ("m", eager._adam["m"], indexed._adam["m"]),
                           ("v", eager._adam["v"], indexed._adam["v"]), ("grad", eager._garena, indexed._garena)):
            assert torch.equal(a, b), (t, name)
