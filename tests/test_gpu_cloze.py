"""BERT4Rec's masking step and cloze head on the GPU (bsarec_cloze_mask, bsarec_cloze_head_fwd / _bwd): the mask kernels equal to
the fp64/integer restatement (cloze_ref) element for element, the head against the fp64 reference at the gates of
test_gpu_ce_head, and the head's identities: the plain head's bits with an identity list, exact zeros outside the list,
determinism, and dead entries never read."""
import functools

import numpy as np
import pytest

from conftest import rel_l2
import cloze_ref as R

pytestmark = pytest.mark.gpu
G = 0.37
SEED = 0x1234567


def _ids(B, L, V, seed):
    """Left-padded rows of mixed lengths: row 0 all padding (where B > 1), row 1 full, the rest random."""
    rng = np.random.default_rng(seed)
    ids = np.zeros((B, L), np.int64)
    for b in range(B):
        n = L if B == 1 else (0 if b == 0 else (L if b == 1 else int(rng.integers(1, L + 1))))
        if n:
            ids[b, L - n:] = rng.integers(1, V, size=n)
    return ids


def _mask(ids_t, ratio, slots, mask_token, state):
    import torch
    from bsarec_amd import _lib
    lib = _lib.load()
    B, L = ids_t.shape
    Rn = B * slots
    masked = torch.full((B, L), -7, dtype=torch.int64, device="cuda")
    rows = torch.full((Rn,), -7, dtype=torch.int32, device="cuda")
    targets = torch.full((Rn,), -7, dtype=torch.int64, device="cuda")
    count = torch.full((1,), -7, dtype=torch.int32, device="cuda")
    _lib.check(lib.bsarec_cloze_mask(ids_t.data_ptr(), B, L, ratio, slots, mask_token, state.data_ptr(), masked.data_ptr(),
                                     rows.data_ptr(), targets.data_ptr(), count.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream), "bsarec_cloze_mask")
    return masked.cpu().numpy(), rows.cpu().numpy(), targets.cpu().numpy(), int(count.item())


MASK_CASES = [(1, 1, 1, 1.0), (3, 50, 20, 0.2), (5, 64, 64, 1.0), (2, 65, 7, 0.5), (4, 256, 30, 0.2), (33, 50, 10, 0.9),
              (6, 50, 20, 0.0)]


@pytest.mark.parametrize("B,L,slots,ratio", MASK_CASES)
def test_mask_kernel_equals_the_reference(B, L, slots, ratio):
    import torch
    V = 131
    ids = _ids(B, L, V, 7 * B + L)
    state = torch.zeros(8, dtype=torch.int64, device="cuda")
    state[0], state[1] = SEED, 5
    ids_t = torch.from_numpy(ids).cuda()
    for step in (5, 6):                              # the second call: state[1] changed, the reference's masks of that step
        state[1] = step
        got = _mask(ids_t, ratio, slots, V, state)
        want = R.cloze_mask(ids, ratio, slots, SEED, step, V)
        assert got[3] == want[3], (step, got[3], want[3])
        for name, g, w in zip(("masked_ids", "rows", "targets"), got, want):
            assert g.dtype == w.dtype and np.array_equal(g, w), (step, name)
        assert int(state[1].item()) == step          # read, not advanced
        n = want[3]
        if B > 1:
            assert not (want[1][:n] // L == 0).any()             # the all-padding row gives nothing
            assert (want[1][:n] // L == 1).any()                 # the full row gives at least one
    if 0.0 < ratio < 1.0 and B * L >= 100:
        assert not np.array_equal(R.cloze_mask(ids, ratio, slots, SEED, 5, V)[0], R.cloze_mask(ids, ratio, slots, SEED, 6, V)[0])


def _head(h, E, rows, targets, count, T, V, g=G, want_rows=True):
    """loss, rows_out, dh, dE through the ctypes bindings; E may have more than V rows."""
    import torch
    from bsarec_amd import _lib
    lib = _lib.load()
    d, Rn = h.shape[1], rows.shape[0]
    nb = lib.bsarec_cloze_head_workspace_bytes(Rn, V, d)
    assert nb == lib.bsarec_ce_head_workspace_bytes(Rn, V, d) > 0
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    loss = torch.full((1,), float("nan"), device="cuda")
    out_rows = torch.full((Rn,), float("nan"), device="cuda") if want_rows else None
    dh, dE = torch.full((T, d), float("nan"), device="cuda"), torch.full((V, d), float("nan"), device="cuda")
    gout = torch.full((1,), g, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.bsarec_cloze_head_fwd(h.data_ptr(), h.stride(0), T, E.data_ptr(), Rn, V, d, rows.data_ptr(), targets.data_ptr(),
                                         count.data_ptr(), loss.data_ptr(), out_rows.data_ptr() if want_rows else None,
                                         ws.data_ptr(), nb, st), "bsarec_cloze_head_fwd")
    _lib.check(lib.bsarec_cloze_head_bwd(h.data_ptr(), h.stride(0), T, E.data_ptr(), Rn, V, d, rows.data_ptr(), targets.data_ptr(),
                                         count.data_ptr(), gout.data_ptr(), ws.data_ptr(), nb, dh.data_ptr(), dE.data_ptr(), st),
               "bsarec_cloze_head_bwd")
    return loss, out_rows, dh, dE


@functools.lru_cache(maxsize=None)
def _case(Rn, n, T, V, d):
    """fp32-rounded inputs, a row list scattered over T (ascending, distinct), and the fp64 reference -- computed once."""
    rng = np.random.default_rng(1009 * Rn + 17 * n + T + V + d)
    h = rng.normal(0, 1, (T, d)).astype(np.float32)
    E = rng.normal(0, 1 / np.sqrt(d), (V + 1, d)).astype(np.float32)          # one row more than the classes: the mask token's
    rows = np.full(Rn, -1, np.int32)
    rows[:n] = np.sort(rng.choice(T, size=n, replace=False))
    targets = np.zeros(Rn, np.int64)
    targets[:n] = rng.integers(0, V, n)
    if n > 1:
        targets[0], targets[1] = 0, V - 1
    return h, E, rows, targets, R.cloze_head(h, E[:V], rows, targets, n, G)


def _gpu(*arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in arrays]


HEAD_SHAPES = [(8, 1, 8, 1, 4), (200, 150, 250, 131, 64), (200, 0, 250, 131, 64), (256, 256, 300, 300, 32), (64, 40, 100, 129, 256)]


@pytest.mark.parametrize("Rn,n,T,V,d", HEAD_SHAPES)
def test_head_vs_fp64_reference(Rn, n, T, V, d):
    """Gates (those of test_gpu_ce_head: the same kernels, the same arithmetic): loss 5e-6 rel, rows 1e-5 abs, dh and dE 1e-4
    rel-L2."""
    import torch
    h, E, rows, targets, (rloss, rrows, rdh, rdE) = _case(Rn, n, T, V, d)
    th, tE, trows, ttargets = _gpu(h, E, rows, targets)
    count = torch.tensor([n], dtype=torch.int32, device="cuda")
    loss, out_rows, dh, dE = _head(th, tE, trows, ttargets, count, T, V)
    loss, out_rows, dh, dE = loss.item(), out_rows.cpu().numpy().astype(np.float64), dh.cpu().numpy(), dE.cpu().numpy()
    e_loss = abs(loss - rloss) / abs(rloss) if rloss != 0 else abs(loss)
    e_rows = np.abs(out_rows - rrows).max()
    e_dh = rel_l2(dh, rdh) if n and V > 1 else float(np.abs(dh).max())
    e_dE = rel_l2(dE, rdE) if n and V > 1 else float(np.abs(dE).max())
    print(f"cloze_head R={Rn} n={n} T={T} V={V} d={d}: loss {loss:.7f} rel {e_loss:.2e} rows {e_rows:.2e} dh {e_dh:.2e} dE {e_dE:.2e}")
    assert np.isfinite(dh).all() and np.isfinite(dE).all()
    assert e_loss <= 5e-6
    assert e_rows <= 1e-5
    assert e_dh <= 1e-4
    assert e_dE <= 1e-4
    assert not out_rows[n:].any()                                # 0 behind the live rows
    outside = np.ones(T, bool)
    outside[rows[:n]] = False
    assert not dh[outside].any()                                 # rows of dh outside the list: exactly 0
    if n == 0 or V == 1:
        assert loss == 0.0 and not dh.any() and not dE.any()


def test_identity_list_gives_the_bits_of_the_plain_head():
    import torch
    from bsarec_amd import _lib
    lib = _lib.load()
    B, V, d = 200, 131, 64
    rng = np.random.default_rng(5)
    h = rng.normal(0, 1, (B, d)).astype(np.float32)
    E = rng.normal(0, 1 / 8, (V, d)).astype(np.float32)
    a = rng.integers(0, V, B).astype(np.int64)
    th, tE, ta = _gpu(h, E, a)
    rows = torch.arange(B, dtype=torch.int32, device="cuda")
    count = torch.tensor([B], dtype=torch.int32, device="cuda")
    loss, out_rows, dh, dE = _head(th, tE, rows, ta, count, B, V)
    nb = lib.bsarec_ce_head_workspace_bytes(B, V, d)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    loss2, rows2 = torch.empty(1, device="cuda"), torch.empty(B, device="cuda")
    dh2, dE2 = torch.empty(B, d, device="cuda"), torch.empty(V, d, device="cuda")
    gout = torch.full((1,), G, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.bsarec_ce_head_fwd(th.data_ptr(), d, tE.data_ptr(), B, V, d, ta.data_ptr(), loss2.data_ptr(), rows2.data_ptr(),
                                      ws.data_ptr(), nb, st), "bsarec_ce_head_fwd")
    _lib.check(lib.bsarec_ce_head_bwd(th.data_ptr(), d, tE.data_ptr(), B, V, d, ta.data_ptr(), gout.data_ptr(), ws.data_ptr(), nb,
                                      dh2.data_ptr(), dE2.data_ptr(), st), "bsarec_ce_head_bwd")
    assert torch.equal(loss, loss2) and torch.equal(out_rows, rows2) and torch.equal(dh, dh2) and torch.equal(dE, dE2)


def test_two_runs_give_equal_bits_and_dead_entries_are_not_read():
    import torch
    Rn, n, T, V, d = 200, 150, 250, 131, 64
    h, E, rows, targets, _ = _case(Rn, n, T, V, d)
    th, tE, trows, ttargets = _gpu(h, E, rows, targets)
    count = torch.tensor([n], dtype=torch.int32, device="cuda")
    first = _head(th, tE, trows, ttargets, count, T, V)
    second = _head(th, tE, trows, ttargets, count, T, V)
    for x, y in zip(first, second):
        assert torch.equal(x, y)
    rows2, targets2 = rows.copy(), targets.copy()
    rows2[n:] = np.arange(Rn - n) % T                            # other IN-RANGE values behind the live rows
    targets2[n:] = 5
    trows2, ttargets2 = _gpu(rows2, targets2)
    third = _head(th, tE, trows2, ttargets2, count, T, V)
    for x, y in zip(first, third):
        assert torch.equal(x, y)
    big = torch.tensor([Rn + 1000], dtype=torch.int32, device="cuda")         # a count above the capacity is the capacity
    full_rows = np.sort(np.random.default_rng(1).choice(T, size=Rn, replace=False)).astype(np.int32)
    tfr = _gpu(full_rows)[0]
    a = _head(th, tE, tfr, ttargets2, big, T, V)
    b = _head(th, tE, tfr, ttargets2, torch.tensor([Rn], dtype=torch.int32, device="cuda"), T, V)
    for x, y in zip(a, b):
        assert torch.equal(x, y)


def test_mask_feeds_the_head():
    """The two calls chained as the model chains them: the mask's rows, targets and count straight into the head."""
    import torch
    B, L, V, d, slots = 9, 50, 131, 64, 20
    ids = _ids(B, L, V, 3)
    state = torch.zeros(8, dtype=torch.int64, device="cuda")
    state[0], state[1] = SEED, 9
    from bsarec_amd import _lib
    lib = _lib.load()
    ids_t = torch.from_numpy(ids).cuda()
    masked = torch.empty_like(ids_t)
    rows = torch.empty(B * slots, dtype=torch.int32, device="cuda")
    targets = torch.empty(B * slots, dtype=torch.int64, device="cuda")
    count = torch.empty(1, dtype=torch.int32, device="cuda")
    _lib.check(lib.bsarec_cloze_mask(ids_t.data_ptr(), B, L, 0.2, slots, V, state.data_ptr(), masked.data_ptr(), rows.data_ptr(),
                                     targets.data_ptr(), count.data_ptr(), torch.cuda.current_stream().cuda_stream), "mask")
    rng = np.random.default_rng(4)
    h = rng.normal(0, 1, (B * L, d)).astype(np.float32)
    E = rng.normal(0, 1 / 8, (V + 1, d)).astype(np.float32)
    th, tE = _gpu(h, E)
    loss, out_rows, dh, dE = _head(th, tE, rows, targets, count, B * L, V)
    _, rrows, rtargets, n = R.cloze_mask(ids, 0.2, slots, SEED, 9, V)
    rloss, _, rdh, rdE = R.cloze_head(h, E[:V], rrows, rtargets, n, G)
    assert 0 < n < B * slots
    assert abs(loss.item() - rloss) <= 5e-6 * abs(rloss)
    assert rel_l2(dh.cpu().numpy(), rdh) <= 1e-4 and rel_l2(dE.cpu().numpy(), rdE) <= 1e-4
