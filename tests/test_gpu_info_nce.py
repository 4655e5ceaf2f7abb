"""DuoRec's HIP contrastive head on the GPU (bsarec_info_nce_fwd / _bwd, DuoRecModel(duorec_head='hip')): the kernels against
the fp64 restatement (info_nce_ref), saturated and degenerate rows, strided views, determinism, graph capture, and the model
against the reference golden and against its own torch head."""
import argparse
import functools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, rel_l2
import info_nce_ref as R

pytestmark = pytest.mark.gpu
G = 0.37


def _call(zi, zj, tau, sim, g=G, rows=True):
    """loss, rows, dz_i, dz_j (torch tensors on the GPU) through the ctypes bindings, on the current stream."""
    import torch
    from bsarec_amd import _lib
    lib = _lib.load()
    B, d = zi.shape
    s = 1 if sim == "cos" else 0
    nb = lib.bsarec_info_nce_workspace_bytes(B, d, s)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    loss = torch.full((1,), float("nan"), device="cuda")
    out_rows = torch.full((2 * B,), float("nan"), device="cuda") if rows else None
    dzi, dzj = torch.full((B, d), float("nan"), device="cuda"), torch.full((B, d), float("nan"), device="cuda")
    gout = torch.full((1,), g, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.bsarec_info_nce_fwd(zi.data_ptr(), zi.stride(0), zj.data_ptr(), zj.stride(0), B, d, 1.0 / tau, s, loss.data_ptr(),
                                       out_rows.data_ptr() if rows else None, ws.data_ptr(), nb, st), "bsarec_info_nce_fwd")
    _lib.check(lib.bsarec_info_nce_bwd(zi.data_ptr(), zi.stride(0), zj.data_ptr(), zj.stride(0), B, d, 1.0 / tau, s, gout.data_ptr(),
                                       ws.data_ptr(), nb, dzi.data_ptr(), dzj.data_ptr(), st), "bsarec_info_nce_bwd")
    return loss, out_rows, dzi, dzj


@functools.lru_cache(maxsize=None)
def _case(B, d, sim, tau, kind="plain"):
    """fp32-rounded inputs and their fp64 reference, computed once per case."""
    rng = np.random.default_rng(1000 * B + d)
    sd = {"plain": 1.0 if sim == "cos" else 0.3, "saturated": 1.3, "degenerate": 1.0}[kind]
    zi, zj = (rng.normal(0, sd, (B, d)).astype(np.float32) for _ in range(2))
    if kind == "degenerate":
        zi[3] = 0.0                                                       # an all-zero row
        zj[5] *= np.float32(1e-9 / np.linalg.norm(zj[5].astype(np.float64)))     # a row of norm 1e-9, below the clamp
    return zi, zj, R.info_nce(zi, zj, tau, sim, G)


def _run_case(B, d, sim, tau, kind="plain"):
    import torch
    zi, zj, ref = _case(B, d, sim, tau, kind)
    loss, rows, dzi, dzj = _call(torch.from_numpy(zi).cuda(), torch.from_numpy(zj).cuda(), tau, sim)
    return ref, (loss.item(), rows.cpu().numpy().astype(np.float64), dzi.cpu().numpy(), dzj.cpu().numpy())


# every B at d = 64, every d at B = 33; then shapes whose workgroups walk SEVERAL key tiles (n / 64 = T > 8 row tiles, S = 8
# splits: B = 300 gives T = 10, B = 1024 gives T = 32 and n > 1024 rows for the one-workgroup statistics pass), at d = 64 and
# at d = 160 (three 64-column chunks: the row tile is staged again per key tile, and nce_bwd_kernel<3>)
SHAPES = ([(B, 64) for B in (1, 2, 33, 64, 65, 256)] + [(33, d) for d in (4, 100, 256)] +
          [(300, 64), (1024, 64), (33, 160), (300, 160)])


@pytest.mark.parametrize("tau", [1.0, 0.2])
@pytest.mark.parametrize("sim", ["dot", "cos"])
@pytest.mark.parametrize("B,d", SHAPES)
def test_kernel_vs_fp64_reference(B, d, sim, tau):
    """Gates: loss 5e-6 rel, dz_i and dz_j 1e-4 rel-L2 each (tests/test_duorec.py), rows_out 1e-5 abs."""
    (rloss, rrows, rdzi, rdzj), (loss, rows, dzi, dzj) = _run_case(B, d, sim, tau)
    e_loss = abs(loss - rloss) / abs(rloss) if rloss != 0 else abs(loss)
    e_rows, e_i, e_j = np.abs(rows - rrows).max(), rel_l2(dzi, rdzi), rel_l2(dzj, rdzj)
    print(f"info_nce B={B} d={d} {sim} tau={tau}: loss {loss:.7f} rel {e_loss:.2e} rows {e_rows:.2e} dz_i {e_i:.2e} dz_j {e_j:.2e}")
    if B == 1:
        assert loss == 0.0 and not rows.any() and not dzi.any() and not dzj.any()      # exactly
    assert e_loss <= 5e-6
    assert e_rows <= 1e-5
    assert e_i <= 1e-4 and e_j <= 1e-4


def test_saturated_scores_stay_finite():
    """dot, rows N(0, 1.3^2), d = 64, B = 33, tau = 1: the self scores |z_r|^2 are about 108 > 88, where expf overflows (the
    diagonal is excluded from the sums: a kernel that exponentiates before it masks, or without the maximum subtracted, gets
    inf or NaN).  tau = 1 and not 0.2: there the row losses pass 128, where half an fp32 ulp is 7.6e-6 and a gate of 1e-5 abs
    says nothing about a kernel whose outputs are fp32."""
    (rloss, rrows, rdzi, rdzj), (loss, rows, dzi, dzj) = _run_case(33, 64, "dot", 1.0, "saturated")
    zi, zj, _ = _case(33, 64, "dot", 1.0, "saturated")
    assert np.median((np.concatenate([zi, zj]).astype(np.float64) ** 2).sum(1)) > 88
    e_rows, e_dz = np.abs(rows - rrows).max(), max(np.abs(dzi - rdzi).max(), np.abs(dzj - rdzj).max())
    print(f"info_nce saturated: loss {loss:.6f} (ref {rloss:.6f}) rows max {rrows.max():.2f} err {e_rows:.2e} dz abs err {e_dz:.2e}")
    assert np.isfinite(loss) and np.isfinite(rows).all() and np.isfinite(dzi).all() and np.isfinite(dzj).all()
    assert e_rows <= 1e-5
    assert e_dz <= 1e-6


@pytest.mark.parametrize("tau", [1.0, 0.2])
def test_cos_zero_row_and_row_below_the_clamp(tau):
    B = 33
    (rloss, rrows, rdzi, rdzj), (loss, rows, dzi, dzj) = _run_case(B, 64, "cos", tau, "degenerate")
    e_rows = np.abs(rows - rrows).max()
    e_zero, e_tiny = rel_l2(dzi[3], rdzi[3]), rel_l2(dzj[5], rdzj[5])
    keep_i, keep_j = np.arange(B) != 3, np.arange(B) != 5
    e_i, e_j = rel_l2(dzi[keep_i], rdzi[keep_i]), rel_l2(dzj[keep_j], rdzj[keep_j])
    print(f"info_nce degenerate tau={tau}: rows {e_rows:.2e} zero row {e_zero:.2e} (|dz| {np.linalg.norm(rdzi[3]):.2e}) "
          f"tiny row {e_tiny:.2e} (|dz| {np.linalg.norm(rdzj[5]):.2e}) rest {e_i:.2e} {e_j:.2e}")
    assert np.linalg.norm(rdzi[3]) > 1e4 and np.linalg.norm(rdzj[5]) > 1e4          # gradients through 1 / 1e-8
    assert e_rows <= 1e-5
    assert e_zero <= 1e-4 and e_tiny <= 1e-4
    assert e_i <= 1e-4 and e_j <= 1e-4
    assert abs(loss - rloss) <= 5e-6 * abs(rloss)


@pytest.mark.parametrize("sim", ["dot", "cos"])
def test_strided_views_and_determinism(sim):
    """[:, -1, :] views of a [B, 50, d] tensor (row stride 50 d) give the bits of their contiguous copies; two runs agree."""
    import torch
    B, d = 65, 64
    g = torch.Generator(device="cuda").manual_seed(5)
    full_i, full_j = (torch.randn(B, 50, d, device="cuda", generator=g) * 0.3 for _ in range(2))
    vi, vj = full_i[:, -1, :], full_j[:, -1, :]
    assert vi.stride(0) == 50 * d and not vi.is_contiguous()
    a = _call(vi, vj, 0.2, sim)
    b = _call(vi.contiguous(), vj.contiguous(), 0.2, sim)
    c = _call(vi, vj, 0.2, sim)
    for x, y, z in zip(a, b, c):
        assert torch.equal(x, y) and torch.equal(x, z)
        assert torch.isfinite(x).all()


def test_forward_and_backward_replay_in_a_graph():
    """Forward + backward captured once on static buffers; the replay after z and gout were overwritten in place equals the
    eager result on the new values bit for bit."""
    import torch
    from bsarec_amd import _lib
    lib = _lib.load()
    B, d, tau = 33, 64, 0.2
    gen = torch.Generator(device="cuda").manual_seed(9)
    zi, zj = (torch.randn(B, d, device="cuda", generator=gen) for _ in range(2))
    gout = torch.full((1,), 1.0, device="cuda")
    nb = lib.bsarec_info_nce_workspace_bytes(B, d, 1)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    loss, rows = torch.zeros(1, device="cuda"), torch.zeros(2 * B, device="cuda")
    dzi, dzj = torch.zeros(B, d, device="cuda"), torch.zeros(B, d, device="cuda")

    def both():
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(lib.bsarec_info_nce_fwd(zi.data_ptr(), d, zj.data_ptr(), d, B, d, 1.0 / tau, 1, loss.data_ptr(), rows.data_ptr(),
                                           ws.data_ptr(), nb, st), "bsarec_info_nce_fwd")
        _lib.check(lib.bsarec_info_nce_bwd(zi.data_ptr(), d, zj.data_ptr(), d, B, d, 1.0 / tau, 1, gout.data_ptr(), ws.data_ptr(), nb,
                                           dzi.data_ptr(), dzj.data_ptr(), st), "bsarec_info_nce_bwd")

    both()                                                    # first launches (code object load) outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    zi.copy_(torch.randn(B, d, device="cuda", generator=gen))
    zj.copy_(torch.randn(B, d, device="cuda", generator=gen))
    gout.fill_(G)
    for t in (loss, rows, dzi, dzj):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    want = _call(zi, zj, tau, "cos")
    for got, w in zip((loss, rows, dzi, dzj), want):
        assert torch.equal(got, w)
    assert float(dzi.abs().max()) > 0


def _golden():
    z = np.load(os.path.join(GOLDEN, "duorec_A_d64_L50_h2.npz"))
    return z, json.loads(str(z["cfg"]))


def test_hip_head_duorec_vs_reference_golden():
    """The body of test_duorec.test_hip_duorec_vs_reference_golden with duorec_head = 'hip' (us_x, dot, tau = 1), at its gates."""
    import torch
    from bsarec_amd import DuoRecModel
    z, cfg = _golden()
    a = argparse.Namespace(hidden_act="gelu", batch_size=10, c=3, seed=1, duorec_head="hip", **cfg)
    m = DuoRecModel(a)
    keys = [k[2:] for k in z.files if k.startswith("p/")]
    m.load_state_dict({k: torch.from_numpy(z["p/" + k]) for k in keys})
    m = m.cuda()
    m.train()
    ids, sem, ans = (torch.from_numpy(z[k]).cuda() for k in ("ids", "sem", "answers"))
    loss = m.calculate_loss(ids, ans, None, sem, None)
    print(f"hip head golden: loss {loss.item():.7f} ref {float(z['loss']):.7f}")
    assert abs(loss.item() - float(z["loss"])) <= 5e-6 * abs(float(z["loss"]))
    m.zero_grad()
    loss.backward()
    grads = {}
    for name, p in m.named_parameters():
        rk = DuoRecModel._ref_key(name)
        if rk is None:
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            continue
        grads[rk] = p.grad.cpu().numpy()
    assert len(keys) == 36
    for k in keys:
        if k.endswith("key.bias"):
            assert np.abs(grads[k]).max() <= 1e-6
            continue
        assert rel_l2(grads[k], z["g/" + k]) <= 1e-4, (k, rel_l2(grads[k], z["g/" + k]))
    assert len(m._slots_busy) == 0
    opt = torch.optim.Adam(m.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=0.0)
    losses = []
    for _ in range(3):
        l = m.calculate_loss(ids, ans, None, sem, None)
        opt.zero_grad()
        l.backward()
        opt.step()
        losses.append(l.item())
    np.testing.assert_allclose(losses, z["adam_losses"], rtol=1e-5)
    sd = m.state_dict()
    for k in keys:
        got, want = sd[k].cpu().numpy(), z["a/" + k]
        if k.endswith("key.bias"):
            continue
        bad = np.abs(got - want) > 2e-5
        assert bad.mean() <= 2e-3, (k, bad.mean(), np.abs(got - want).max())


@pytest.fixture(scope="module")
def two_heads():
    """The golden's parameters and shapes with dropout on, once per head.  Every test runs both models through the same
    calls, so their dropout step counters stay equal."""
    import torch
    from bsarec_amd import DuoRecModel
    z, cfg = _golden()
    cfg = dict(cfg, hidden_dropout_prob=0.3, attention_probs_dropout_prob=0.2)
    keys = [k[2:] for k in z.files if k.startswith("p/")]
    models = {}
    for head in ("torch", "hip"):
        m = DuoRecModel(argparse.Namespace(hidden_act="gelu", batch_size=10, c=3, seed=1, duorec_head=head, **cfg))
        m.load_state_dict({k: torch.from_numpy(z["p/" + k]) for k in keys})
        models[head] = m.cuda().train()
    return models, tuple(torch.from_numpy(z[k]).cuda() for k in ("ids", "sem", "answers"))


@pytest.mark.parametrize("sim", ["dot", "cos"])
@pytest.mark.parametrize("ssl", ["us", "un", "su", "us_x"])
def test_hip_head_vs_torch_head(two_heads, ssl, sim):
    """Same seed, same dropout masks: loss 5e-6 rel, every gradient 1e-4 rel-L2 (key.bias, whose gradient is zero in exact
    arithmetic, 1e-6 abs as in the golden test)."""
    models, (ids, sem, ans) = two_heads
    out = {}
    for head, m in models.items():
        m.ssl, m.sim = ssl, sim
        m.set_seed(123)
        m.zero_grad()
        loss = m.calculate_loss(ids, ans, None, sem, None)
        loss.backward()
        assert len(m._slots_busy) == 0
        out[head] = (loss.item(), {n: p.grad.cpu().numpy().copy() for n, p in m.named_parameters() if p.grad is not None})
    (lt, gt), (lh, gh) = out["torch"], out["hip"]
    print(f"heads {ssl} {sim}: torch {lt:.7f} hip {lh:.7f}")
    assert abs(lh - lt) <= 5e-6 * abs(lt)
    assert gt.keys() == gh.keys() and len(gt) >= 36
    worst = 0.0
    for n in gt:
        if n.endswith("key.bias"):
            assert np.abs(gh[n]).max() <= 1e-6 and np.abs(gt[n]).max() <= 1e-6
            continue
        if not gt[n].any() and not gh[n].any():
            continue                                           # the unused frequency branch
        e = rel_l2(gh[n], gt[n])
        worst = max(worst, e)
        assert e <= 1e-4, (n, e)
    print(f"heads {ssl} {sim}: worst gradient rel-L2 {worst:.2e}")
