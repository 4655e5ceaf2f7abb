"""The HIP full-catalogue cross-entropy head on the GPU (bsarec_ce_head_fwd / _bwd, BSARecModel.catalogue_ce,
DuoRecModel(duorec_ce_head='hip')): the kernels against the fp64 restatement (ce_head_ref), saturated scores, V = 1, strided
views, determinism, graph capture, peak memory, and the model against the reference golden and against its own torch head."""
import argparse
import functools
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, rel_l2
import ce_head_ref as R

pytestmark = pytest.mark.gpu
G = 0.37


def _call(h, E, a, g=G, rows=True):
    """loss, rows, dh, dE (torch tensors on the GPU) through the ctypes bindings, on the current stream."""
    import torch
    from bsarec_amd import _lib
    lib = _lib.load()
    (B, d), V = h.shape, E.shape[0]
    nb = lib.bsarec_ce_head_workspace_bytes(B, V, d)
    assert 0 < nb <= (16384 + 2 * B) * (d + 8) * 4
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    loss = torch.full((1,), float("nan"), device="cuda")
    out_rows = torch.full((B,), float("nan"), device="cuda") if rows else None
    dh, dE = torch.full((B, d), float("nan"), device="cuda"), torch.full((V, d), float("nan"), device="cuda")
    gout = torch.full((1,), g, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.bsarec_ce_head_fwd(h.data_ptr(), h.stride(0), E.data_ptr(), B, V, d, a.data_ptr(), loss.data_ptr(),
                                      out_rows.data_ptr() if rows else None, ws.data_ptr(), nb, st), "bsarec_ce_head_fwd")
    _lib.check(lib.bsarec_ce_head_bwd(h.data_ptr(), h.stride(0), E.data_ptr(), B, V, d, a.data_ptr(), gout.data_ptr(),
                                      ws.data_ptr(), nb, dh.data_ptr(), dE.data_ptr(), st), "bsarec_ce_head_bwd")
    return loss, out_rows, dh, dE


def _answers(rng, B, V):
    """Uniform, then forced: item 0, item V - 1, the first item of the last (partial) 128-item tile, one id shared by two rows."""
    a = rng.integers(0, V, B)
    a[0] = 0
    if B > 1:
        a[1] = V - 1
    if B > 2:
        a[2] = (V - 1) // 128 * 128
    if B > 4:
        a[4] = a[3]
    return a.astype(np.int64)


@functools.lru_cache(maxsize=None)
def _case(B, V, d, scale=1.0):
    """fp32-rounded inputs and their fp64 reference, computed once per case."""
    rng = np.random.default_rng(100003 * B + 101 * V + d)
    h = (rng.normal(0, 1, (B, d)) * scale).astype(np.float32)
    E = rng.normal(0, 1 / np.sqrt(d), (V, d)).astype(np.float32)
    a = _answers(rng, B, V)
    if scale != 1.0:                                          # saturated: the answer is the row maximum for half the rows
        s = h.astype(np.float64) @ E.astype(np.float64).T
        a[B // 2:] = s[B // 2:].argmax(1)
    return h, E, a, R.ce_head(h, E, a, G)


def _gpu(*arrays):
    import torch
    return [torch.from_numpy(x).cuda() for x in arrays]


def _errors(ref, got, a, V):
    (rloss, rrows, rdh, rdE), (loss, rows, dh, dE) = ref, got
    loss, rows, dh, dE = loss.item(), rows.cpu().numpy().astype(np.float64), dh.cpu().numpy(), dE.cpu().numpy()
    e_loss = abs(loss - rloss) / abs(rloss) if rloss != 0 else abs(loss)
    rest = np.ones(V, bool)
    rest[a] = False
    e_rest = rel_l2(dE[rest], rdE[rest]) if rest.any() else 0.0
    return loss, rows, dh, dE, e_loss, np.abs(rows - rrows).max(), rel_l2(dh, rdh), rel_l2(dE, rdE), e_rest


# every B at (V, d) = (1000, 64), every V at (B, d) = (33, 64), every d at (B, V) = (33, 1000); then two shapes in which a
# workgroup walks several item tiles, several V splits merge (547 item blocks), the dE loop crosses several row tiles of 128, and
# the last tiles are partial on both axes: d = 64 (ce_dh_kernel<4, 2>) and d = 160 (ce_dh_kernel<1, 8>, 32-row tiles)
SHAPES = ([(B, 1000, 64) for B in (1, 2, 33, 64, 65)] + [(33, V, 64) for V in (1, 2, 63, 64, 65, 129, 4099)] +
          [(33, 1000, d) for d in (4, 100, 160, 256)] + [(300, 70001, 64), (130, 70001, 160)])


@pytest.mark.parametrize("B,V,d", SHAPES)
def test_kernel_vs_fp64_reference(B, V, d):
    """Gates: loss 5e-6 rel, rows_out 1e-5 abs, dh 1e-4 rel-L2, dE 1e-4 rel-L2 over the whole table and, separately, over
    the rows that are nobody's answer."""
    h, E, a, ref = _case(B, V, d)
    loss, rows, dh, dE, e_loss, e_rows, e_dh, e_dE, e_rest = _errors(ref, _call(*_gpu(h, E, a)), a, V)
    print(f"ce_head B={B} V={V} d={d}: loss {loss:.7f} rel {e_loss:.2e} rows {e_rows:.2e} dh {e_dh:.2e} dE {e_dE:.2e} "
          f"dE(non-answer rows) {e_rest:.2e}")
    if V == 1:
        assert loss == 0.0 and not rows.any() and not dh.any() and not dE.any()        # exactly
    assert np.isfinite(dh).all() and np.isfinite(dE).all()
    assert e_loss <= 5e-6
    assert e_rows <= 1e-5
    assert e_dh <= 1e-4
    assert e_dE <= 1e-4 and e_rest <= 1e-4


def test_b1_v1_is_exactly_zero():
    h, E, a, ref = _case(1, 1, 64)
    loss, rows, dh, dE = _call(*_gpu(h, E, a))
    assert loss.item() == 0.0 and rows.item() == 0.0 and not dh.any().item() and not dE.any().item()
    assert ref[0] == 0.0


def test_saturated_scores_against_the_torch_head():
    """h scaled by 40: the row maxima of |s| have a median above 88, where expf overflows without the maximum subtracted.  The
    rounding of s itself has no a-priori bound here, so each error of the HIP head against the fp64 reference (rows, dh, dE:
    largest absolute error) is gated at twice the same error of the fp32 torch head (matmul + cross_entropy + autograd, same
    GPU, same inputs) plus 1e-6: two fp32 sums in different orders over the same condition number."""
    import torch
    B, V, d = 32, 1000, 64
    h, E, a, ref = _case(B, V, d, 40.0)
    s = h.astype(np.float64) @ E.astype(np.float64).T
    assert np.median(np.abs(s).max(1)) > 88
    assert (s.argmax(1) == a).sum() >= B // 2
    th, tE, ta = _gpu(h, E, a)
    loss, rows, dh, dE = _call(th, tE, ta)
    for t in (loss, rows, dh, dE):
        assert torch.isfinite(t).all()
    th.requires_grad_(True), tE.requires_grad_(True)
    trow = torch.nn.functional.cross_entropy(torch.matmul(th, tE.T), ta, reduction="none")
    (G * trow.mean()).backward()
    _, rrows, rdh, rdE = ref
    err = lambda x, r: float(np.abs(x.detach().cpu().numpy().astype(np.float64) - r).max())
    for name, got, want, r in (("rows", rows, trow, rrows), ("dh", dh, th.grad, rdh), ("dE", dE, tE.grad, rdE)):
        e_hip, e_torch = err(got, r), err(want, r)
        print(f"ce_head saturated {name}: hip {e_hip:.3e} torch {e_torch:.3e} (largest |ref| {np.abs(r).max():.3e})")
        assert e_hip <= 2 * e_torch + 1e-6, name


def test_strided_view_and_determinism():
    """The [:, -1, :] view of a [B, 50, d] tensor (row stride 50 d) gives the bits of its contiguous copy; two runs agree."""
    import torch
    B, V, d = 65, 4099, 64
    g = torch.Generator(device="cuda").manual_seed(5)
    full = torch.randn(B, 50, d, device="cuda", generator=g)
    E = torch.randn(V, d, device="cuda", generator=g) / 8
    a = torch.from_numpy(_answers(np.random.default_rng(3), B, V)).cuda()
    v = full[:, -1, :]
    assert v.stride(0) == 50 * d and not v.is_contiguous()
    x, y, z = _call(v, E, a), _call(v.contiguous(), E, a), _call(v, E, a)
    for p, q, r in zip(x, y, z):
        assert torch.equal(p, q) and torch.equal(p, r)
        assert torch.isfinite(p).all()


def test_forward_and_backward_replay_in_a_graph():
    """Forward + backward captured once on static buffers; the replay after h, E and gout were overwritten in place equals the
    eager result on the new values bit for bit."""
    import torch
    from bsarec_amd import _lib
    lib = _lib.load()
    B, V, d = 33, 1000, 64
    gen = torch.Generator(device="cuda").manual_seed(9)
    h, E = torch.randn(B, d, device="cuda", generator=gen), torch.randn(V, d, device="cuda", generator=gen) / 8
    a = torch.from_numpy(_answers(np.random.default_rng(4), B, V)).cuda()
    gout = torch.full((1,), 1.0, device="cuda")
    nb = lib.bsarec_ce_head_workspace_bytes(B, V, d)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    loss, rows = torch.zeros(1, device="cuda"), torch.zeros(B, device="cuda")
    dh, dE = torch.zeros(B, d, device="cuda"), torch.zeros(V, d, device="cuda")

    def both():
        st = torch.cuda.current_stream().cuda_stream
        _lib.check(lib.bsarec_ce_head_fwd(h.data_ptr(), d, E.data_ptr(), B, V, d, a.data_ptr(), loss.data_ptr(), rows.data_ptr(),
                                          ws.data_ptr(), nb, st), "bsarec_ce_head_fwd")
        _lib.check(lib.bsarec_ce_head_bwd(h.data_ptr(), d, E.data_ptr(), B, V, d, a.data_ptr(), gout.data_ptr(), ws.data_ptr(), nb,
                                          dh.data_ptr(), dE.data_ptr(), st), "bsarec_ce_head_bwd")

    both()                                                    # first launches (code object load) outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        both()
    h.copy_(torch.randn(B, d, device="cuda", generator=gen))
    E.copy_(torch.randn(V, d, device="cuda", generator=gen) / 8)
    gout.fill_(G)
    for t in (loss, rows, dh, dE):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    want = _call(h, E, a)
    for got, w in zip((loss, rows, dh, dE), want):
        assert torch.equal(got, w)
    assert float(dh.abs().max()) > 0 and float(dE.abs().max()) > 0


def _golden():
    z = np.load(os.path.join(GOLDEN, "duorec_A_d64_L50_h2.npz"))
    return z, json.loads(str(z["cfg"]))


def _duorec(cfg, z, **kw):
    import torch
    from bsarec_amd import DuoRecModel
    m = DuoRecModel(argparse.Namespace(hidden_act="gelu", batch_size=10, c=3, seed=1, **dict(cfg, **kw)))
    if z is not None:
        keys = [k[2:] for k in z.files if k.startswith("p/")]
        m.load_state_dict({k: torch.from_numpy(z["p/" + k]) for k in keys})
    return m.cuda().train()


def test_peak_memory_has_no_b_by_v_term():
    """(B, V, d) = (512, 50000, 64): catalogue_ce + backward allocate the workspace, dE, dh (and at most a copy of h) -- at
    most workspace + 4 (V d + 2 B d) + 1 MiB, below a quarter of one B x V fp32 matrix; the torch head on the same inputs
    holds at least two such matrices (logits and their gradient)."""
    import torch
    from bsarec_amd import _lib
    B, V, d = 512, 50000, 64
    _, cfg = _golden()
    assert cfg["hidden_size"] == d
    m = _duorec(cfg, None, item_size=V)
    W = m.item_embeddings.weight
    assert tuple(W.shape) == (V, d)
    gen = torch.Generator(device="cuda").manual_seed(2)
    h = torch.randn(B, d, device="cuda", generator=gen).requires_grad_(True)
    a = torch.randint(0, V, (B,), device="cuda", generator=gen)
    ws = _lib.load().bsarec_ce_head_workspace_bytes(B, V, d)

    def peak(fn):
        m.zero_grad(set_to_none=True)
        h.grad = None
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        loss = fn()
        loss.backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, loss.item()

    p_hip, l_hip = peak(lambda: m.catalogue_ce(h, a))
    m._ce_pool.clear()
    p_torch, l_torch = peak(lambda: torch.nn.functional.cross_entropy(torch.matmul(h, W.T), a))
    print(f"ce_head peak memory above the inputs at B={B} V={V} d={d}: hip {p_hip / 1e6:.2f} MB (workspace {ws / 1e6:.2f} MB) "
          f"torch {p_torch / 1e6:.2f} MB; B V 4 = {B * V * 4 / 1e6:.1f} MB")
    assert abs(l_hip - l_torch) <= 5e-6 * abs(l_torch)
    assert p_hip <= ws + 4 * (V * d + 2 * B * d) + (1 << 20)
    assert p_hip < B * V * 4 / 4
    assert p_torch >= 2 * B * V * 4


def test_catalogue_ce_autograd():
    """Gradients to seq_output (a [:, -1, :] view) and to item_embeddings.weight against the torch expression: loss 5e-6 rel,
    gradients 1e-4 rel-L2; a second backward raises."""
    import torch
    z, cfg = _golden()
    m = _duorec(cfg, z)
    W = m.item_embeddings.weight
    V, d = W.shape
    B = 33
    gen = torch.Generator(device="cuda").manual_seed(11)
    full = torch.randn(B, 50, d, device="cuda", generator=gen).requires_grad_(True)
    a = torch.from_numpy(_answers(np.random.default_rng(6), B, V)).cuda()
    out = {}
    for head in ("torch", "hip"):
        m.zero_grad(set_to_none=True)
        full.grad = None
        v = full[:, -1, :]
        loss = m.catalogue_ce(v, a) if head == "hip" else torch.nn.functional.cross_entropy(torch.matmul(v, W.T), a)
        assert loss.dim() == 0
        (G * loss).backward(retain_graph=head == "hip")
        out[head] = (loss.item(), full.grad[:, -1, :].cpu().numpy().copy(), W.grad.cpu().numpy().copy())
        if head == "hip":
            assert not full.grad[:, :-1, :].any().item()
            with pytest.raises(RuntimeError, match="backward ran twice"):
                (G * loss).backward()
    (lt, ht, et), (lh, hh, eh) = out["torch"], out["hip"]
    print(f"catalogue_ce: torch {lt:.7f} hip {lh:.7f} dh {rel_l2(hh, ht):.2e} dE {rel_l2(eh, et):.2e}")
    assert abs(lh - lt) <= 5e-6 * abs(lt)
    assert rel_l2(hh, ht) <= 1e-4 and rel_l2(eh, et) <= 1e-4
    assert len(m._slots_busy) == 0


@pytest.mark.parametrize("nce_head", ["torch", "hip"])
def test_hip_ce_head_duorec_vs_reference_golden(nce_head):
    """The reference golden (us_x, dot, tau = 1) with duorec_ce_head = 'hip', alone and together with duorec_head = 'hip', at
    the gates of test_hip_head_duorec_vs_reference_golden: loss 5e-6 rel, 36 gradients 1e-4 rel-L2, key.bias 1e-6 abs."""
    import torch
    from bsarec_amd import DuoRecModel
    z, cfg = _golden()
    m = _duorec(cfg, z, duorec_ce_head="hip", duorec_head=nce_head)
    keys = [k[2:] for k in z.files if k.startswith("p/")]
    ids, sem, ans = (torch.from_numpy(z[k]).cuda() for k in ("ids", "sem", "answers"))
    loss = m.calculate_loss(ids, ans, None, sem, None)
    print(f"hip CE head golden (contrastive head {nce_head}): loss {loss.item():.7f} ref {float(z['loss']):.7f}")
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
    worst = 0.0
    for k in keys:
        if k.endswith("key.bias"):
            assert np.abs(grads[k]).max() <= 1e-6
            continue
        e = rel_l2(grads[k], z["g/" + k])
        worst = max(worst, e)
        assert e <= 1e-4, (k, e)
    print(f"hip CE head golden (contrastive head {nce_head}): worst gradient rel-L2 {worst:.2e}")
    assert len(m._slots_busy) == 0


@pytest.fixture(scope="module")
def two_ce_heads():
    """The golden's parameters and shapes with dropout on, once per CE head.  Every test runs both models through the same
    calls, so their dropout step counters stay equal."""
    import torch
    z, cfg = _golden()
    cfg = dict(cfg, hidden_dropout_prob=0.3, attention_probs_dropout_prob=0.2)
    models = {head: _duorec(cfg, z, duorec_ce_head=head) for head in ("torch", "hip")}
    return models, tuple(torch.from_numpy(z[k]).cuda() for k in ("ids", "sem", "answers"))


@pytest.mark.parametrize("ssl", ["us", "un", "su", "us_x"])
def test_hip_ce_head_vs_torch_ce_head(two_ce_heads, ssl):
    """Same seed, same dropout masks: loss 5e-6 rel, every gradient 1e-4 rel-L2 (key.bias, whose gradient is zero in exact
    arithmetic, 1e-6 abs as in the golden test)."""
    models, (ids, sem, ans) = two_ce_heads
    out = {}
    for head, m in models.items():
        m.ssl = ssl
        m.set_seed(123)
        m.zero_grad()
        loss = m.calculate_loss(ids, ans, None, sem, None)
        loss.backward()
        assert len(m._slots_busy) == 0
        out[head] = (loss.item(), {n: p.grad.cpu().numpy().copy() for n, p in m.named_parameters() if p.grad is not None})
    (lt, gt), (lh, gh) = out["torch"], out["hip"]
    print(f"CE heads {ssl}: torch {lt:.7f} hip {lh:.7f}")
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
    print(f"CE heads {ssl}: worst gradient rel-L2 {worst:.2e}")
