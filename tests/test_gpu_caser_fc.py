"""fc1 of the Caser step alone (bsarec_caser_fc_fwd / bsarec_caser_fc_bwd, csrc/caser_step.h) against numpy double, forward and
backward, at p = 0 and p = 0.5 with the mask rebuilt from the seed and the step counter read back from the device.

  (B, F, d) = (17, 40, 36)      one past a row tile; d and F no multiple of 16
              (1, 4, 4)         every dimension at its minimum
              (65, 4192, 256)   the widest rows, long K, five row tiles
              (33, 1056, 64)    the feature width of the L = 50, n_h = 16, n_v = 4 model

The ReLU is a discrete choice: the inputs are drawn so that the reference has no |u| < 1e-4 under either mask (asserted; the
generator seeds below are the first from 0 at which that holds, found on the CPU)."""
import functools

import numpy as np
import pytest

from conftest import rel_l2
from oracle import bsarec_oracle as O

pytestmark = pytest.mark.gpu
OUT_GATE, GRAD_GATE = 2e-5, 2e-4
MARGIN = 1e-4
CASES = [(17, 40, 36), (1, 4, 4), (65, 4192, 256), (33, 1056, 64)]
CASE_SEED = {(17, 40, 36): 0, (1, 4, 4): 0, (65, 4192, 256): 4, (33, 1056, 64): 0}
PHILOX_SEED, PHILOX_STEP = 0x1234567_89ABCDEF, 3


def inputs(case, seed=None):
    """z [B, F], fc = W1 [d, F] | b1 [d], ds [B, d] in fp32: z and ds ~ N(0, 1), W1 ~ N(0, 1 / F), b1 ~ N(0, 0.1)."""
    B, F, d = case
    rng = np.random.default_rng(CASE_SEED[case] if seed is None else seed)
    z = rng.normal(0, 1, (B, F)).astype(np.float32)
    fc = np.concatenate([rng.normal(0, 1 / np.sqrt(F), d * F), rng.normal(0, 0.1, d)]).astype(np.float32)
    ds = rng.normal(0, 1, (B, d)).astype(np.float32)
    return z, fc, ds


def mult(case, p, seed=PHILOX_SEED, step=PHILOX_STEP):
    B, F, d = case
    if p <= 0.0:
        return np.ones((B, F))
    return O.dropout_keep(B * F, p, int(seed), int(step), 0).reshape(B, F).astype(np.float64) / (1.0 - p)


def reference(z, fc, ds, m):
    """-> (u, s, dz, dfc) in double."""
    z, fc, ds = (np.asarray(v, np.float64) for v in (z, fc, ds))
    B, F = z.shape
    d = ds.shape[1]
    W, b = fc[:d * F].reshape(d, F), fc[d * F:]
    zd = z * m
    u = zd @ W.T + b
    du = ds * (u > 0)
    return u, np.maximum(u, 0.0), (du @ W) * m, np.concatenate([(du.T @ zd).reshape(-1), du.sum(0)])


@functools.lru_cache(maxsize=None)
def _reference(case, p):
    z, fc, ds = inputs(case)
    out = reference(z, fc, ds, mult(case, p))
    assert np.abs(out[0]).min() >= MARGIN, (case, p, np.abs(out[0]).min())      # a condition on the inputs
    return out


def run(case, z, fc, ds, p, train):
    """The two entries on the current stream -> (s, dz, dfc, workspace as floats, state) as torch tensors."""
    import torch
    from bsarec_amd import _lib
    lib = _lib.load()
    B, F, d = case
    dev = torch.device("cuda")
    zt, fct, dst = (torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (z, fc, ds))
    state = torch.zeros(8, dtype=torch.int64, device=dev)
    state[0], state[1] = PHILOX_SEED, PHILOX_STEP
    nbytes = lib.bsarec_caser_fc_workspace_bytes(B, F, d)
    assert nbytes == 4 * B * F
    ws = torch.full((nbytes // 4,), float("nan"), dtype=torch.float32, device=dev)
    s = torch.full((B, d), float("nan"), dtype=torch.float32, device=dev)
    dz = torch.full((B, F), float("nan"), dtype=torch.float32, device=dev)
    dfc = torch.full((d * F + d,), float("nan"), dtype=torch.float32, device=dev)
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.bsarec_caser_fc_fwd(B, F, d, zt.data_ptr(), fct.data_ptr(), state.data_ptr(), int(train), p, s.data_ptr(),
                                       ws.data_ptr(), nbytes, stream), "bsarec_caser_fc_fwd")
    _lib.check(lib.bsarec_caser_fc_bwd(B, F, d, zt.data_ptr(), fct.data_ptr(), s.data_ptr(), dst.data_ptr(), state.data_ptr(),
                                       int(train), p, dz.data_ptr(), dfc.data_ptr(), ws.data_ptr(), nbytes, stream),
               "bsarec_caser_fc_bwd")
    torch.cuda.synchronize()
    return s, dz, dfc, ws, state


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("case", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_forward_and_backward_against_fp64(case, p):
    import torch
    B, F, d = case
    z, fc, ds = inputs(case)
    s, dz, dfc, ws, state = run(case, z, fc, ds, p, 1)
    st = state.cpu().tolist()
    assert st[0] == PHILOX_SEED and st[1] == PHILOX_STEP and not any(st[2:])    # the entries read the state, they move nothing
    m = mult(case, p, st[0], st[1])
    if p > 0.0:
        assert set(np.unique(m)) <= {0.0, 2.0} and (B * F < 64 or 0.3 < (m > 0).mean() < 0.7)
    u_r, s_r, dz_r, dfc_r = _reference(case, p)
    errs = dict(s=rel_l2(s.cpu().numpy(), s_r), dz=rel_l2(dz.cpu().numpy(), dz_r),
                dW1=rel_l2(dfc[:d * F].cpu().numpy(), dfc_r[:d * F]), db1=rel_l2(dfc[d * F:].cpu().numpy(), dfc_r[d * F:]))
    print(f"caser fc {case} p={p}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()) +
          f"  min|u| {np.abs(u_r).min():.2e} alive {(u_r > 0).mean():.2f}")
    assert errs["s"] <= OUT_GATE
    for k in ("dz", "dW1", "db1"):
        assert errs[k] <= GRAD_GATE, (k, errs[k])
    assert np.array_equal(s.cpu().numpy() > 0, u_r > 0)                         # the ReLU switched where the reference's did
    if p > 0.0:
        # the masked forward leaves zd = z (.) m in the workspace; a product with 0 or 2 is exact
        assert np.array_equal(ws.cpu().numpy().reshape(B, F), z * m.astype(np.float32))
        assert not dz.cpu().numpy()[m == 0].any()
    else:
        assert torch.isnan(ws).all().item()                                     # no mask: the workspace is not touched
    # a second run: the same bits
    s2, dz2, dfc2, _, _ = run(case, z, fc, ds, p, 1)
    assert torch.equal(s, s2) and torch.equal(dz, dz2) and torch.equal(dfc, dfc2)


@pytest.mark.parametrize("case", [(17, 40, 36), (33, 1056, 64)], ids=["17-40-36", "33-1056-64"])
def test_train_0_at_p_half_gives_the_bits_of_p_0(case):
    import torch
    z, fc, ds = inputs(case)
    a = run(case, z, fc, ds, 0.5, 0)
    b = run(case, z, fc, ds, 0.0, 1)
    for x, y in zip(a[:3], b[:3]):
        assert torch.equal(x, y)
    assert torch.isnan(a[3]).all().item()


def test_a_row_alone_has_the_bits_it_has_in_its_batch():
    import torch
    case = (33, 1056, 64)
    z, fc, ds = inputs(case)
    s = run(case, z, fc, ds, 0.0, 1)[0]
    alone = run((1, 1056, 64), z[7:8], fc, ds[7:8], 0.0, 1)[0]
    assert torch.equal(s[7:8], alone)
    # under the mask too, when the row keeps its place in the stream: row 0 of the batch
    s5 = run(case, z, fc, ds, 0.5, 1)[0]
    alone5 = run((1, 1056, 64), z[0:1], fc, ds[0:1], 0.5, 1)[0]
    assert torch.equal(s5[0:1], alone5)
