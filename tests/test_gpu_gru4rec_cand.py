"""The GRU4Rec heads over shared candidates on the GPU against gru4rec_cand_ref in numpy double: the head alone
(bsarec_gru4rec_cand_head) at five shapes with constructed collisions, saturated scores against torch fp32 on the CPU, the whole
step (loss_and_grads, three Adam steps) at shapes 1 and 2 of test_gpu_gru4rec_step, bit determinism with a poisoned workspace,
graph replay against eager calls, the torch-op loss of gru_step = "torch", and main.run end to end.

Head shapes (B, d, V):
  (1, 64, 50)     "in_batch": no row has a negative, exact zeros; "+sampled": one negative
  (2, 36, 50)     d no multiple of 32
  (33, 64, 301)   one past a 32-row tile; one slab ("in_batch") and two ("+sampled", C = 66)
  (65, 256, 40)   the widest rows, one past a 64-row tile; 2 and 3 slabs
  (257, 64, 301)  the products split into 5 ("in_batch", C = 257) and 9 ("+sampled", C = 514) slabs, the last one short"""
import ast
import ctypes as C
import functools
import logging

import numpy as np
import pytest

from conftest import rel_l2
import gru4rec_cand_ref as R
import gru4rec_step_ref as S

pytestmark = pytest.mark.gpu
LOSS_GATE, GRAD_GATE = 5e-6, 2e-4                             # those of test_gpu_gru4rec_step
HEAD_SHAPES = [(1, 64, 50), (2, 36, 50), (33, 64, 301), (65, 256, 40), (257, 64, 301)]
COMBOS = [(l, n) for l in R.LOSSES for n in R.NEGATIVES]
BPREG = 0.7
SEED = 5


@functools.lru_cache(maxsize=None)
def _head_inputs(B, d, V, scale=1.0):
    """s ~ N(0, scale), E ~ N(0, 0.5) (scores of a few units: the sigmoids and softmaxes leave their linear range), and a batch
    with these collisions, as far as B has room for them: rows 0 and 1 share an answer (B >= 3), neg[0] is row 2's answer
    (B = 2: row 1's), neg[1] is row 1's own answer, and the last two negatives are equal."""
    import torch
    g = torch.Generator().manual_seed(100 * B + d)
    s = torch.randn(B, d, generator=g) * scale
    E = torch.randn(V, d, generator=g) * 0.5
    pos = torch.randperm(V - 1, generator=g)[:B] + 1 if B <= V - 1 else torch.randint(1, V, (B,), generator=g)
    neg = torch.randint(1, V, (B,), generator=g)
    if B == 1:
        neg[0] = pos[0] % (V - 1) + 1                         # not the answer
    if B >= 3:
        pos[1] = pos[0]
    if B >= 2:
        neg[0] = pos[2 if B >= 3 else 1]
        neg[1] = pos[1]
    if B >= 4:
        neg[B - 1] = neg[B - 2]
    return s, E, pos, neg


def _head_gpu(s, E, pos, neg, loss, negatives, bpreg=BPREG, poison=False):
    """bsarec_gru4rec_cand_head -> (loss, ds, dEc) as numpy."""
    import torch
    from bsarec_amd import _lib
    lib = _lib.load()
    B, d = s.shape
    head = _lib.Gru4RecHead(_lib.GRU4REC_LOSSES[loss], _lib.GRU4REC_CANDIDATES[negatives], bpreg)
    Cn = B * head.candidates
    nbytes = lib.bsarec_gru4rec_cand_head_workspace_bytes(B, d, head)
    assert nbytes > 0
    sg, Eg, pg, ng = s.cuda().contiguous(), E.cuda().contiguous(), pos.cuda(), neg.cuda()
    ws = torch.full((nbytes,), 0xFF if poison else 0, dtype=torch.uint8, device="cuda")
    out = torch.full((1,), float("nan"), device="cuda")
    ds = torch.full((B, d), float("nan"), device="cuda")
    dEc = torch.full((Cn, d), float("nan"), device="cuda")
    stream = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.bsarec_gru4rec_cand_head(sg.data_ptr(), Eg.data_ptr(), pg.data_ptr(), ng.data_ptr(), B, d, E.shape[0], head,
                                            out.data_ptr(), ds.data_ptr(), dEc.data_ptr(), ws.data_ptr(), nbytes, stream),
               "bsarec_gru4rec_cand_head")
    torch.cuda.synchronize()
    return out.item(), ds.cpu().numpy(), dEc.cpu().numpy()


@pytest.mark.parametrize("loss,negatives", COMBOS)
@pytest.mark.parametrize("B,d,V", HEAD_SHAPES)
def test_head_against_the_reference(B, d, V, loss, negatives):
    s, E, pos, neg = _head_inputs(B, d, V)
    M = R.negative_mask(pos.numpy(), neg.numpy(), negatives)
    m = M.sum(1)
    others = (~M).sum(1) - 1                                  # masked columns beside the row's own
    rl, G, rds, rdEc = R.head(s.numpy(), E.numpy(), pos.numpy(), neg.numpy(), loss, negatives, BPREG)
    gl, ds, dEc = _head_gpu(s, E, pos, neg, loss, negatives, poison=True)
    assert np.isfinite(gl) and np.isfinite(ds).all() and np.isfinite(dEc).all()
    if B == 1 and negatives == "in_batch":
        assert m.max() == 0
        assert gl == 0.0 and not ds.any() and not dEc.any() and rl == 0.0
        return
    # the collisions are there: B = 2 under "in_batch" has room for a negative per row and for nothing else
    assert m.max() > 0
    if B >= 3 or (B == 2 and negatives != "in_batch"):
        assert others.max() > 0
    if B >= 4:
        assert pos[0] == pos[1] and neg[1] == pos[1] and neg[0] == pos[2] and neg[B - 1] == neg[B - 2]
    e =(abs(gl - rl) / abs(rl), rel_l2(ds, rds), rel_l2(dEc, rdEc))
    print(f"cand head {loss} {negatives} B={B} d={d} V={V}: loss {gl:.7f} rel {e[0]:.2e} ds {e[1]:.2e} dEc {e[2]:.2e} "
          f"m {m.min()}..{m.max()}")
    assert e[0] <= LOSS_GATE and e[1] <= GRAD_GATE and e[2] <= GRAD_GATE


@pytest.mark.parametrize("loss", R.LOSSES)
def test_all_answers_equal_gives_exact_zeros(loss):
    import torch
    s, E, pos, neg = _head_inputs(33, 64, 301)
    pos = torch.full_like(pos, 17)
    gl, ds, dEc = _head_gpu(s, E, pos, neg, loss, "in_batch", poison=True)
    assert gl == 0.0 and not ds.any() and not dEc.any()


@pytest.mark.parametrize("loss,negatives", COMBOS)
def test_saturated_scores(loss, negatives):
    """s x 50: scores of hundreds.  Finite outputs, and each tensor within 8 x the error that the same formulas make in torch
    fp32 on the CPU (the margin of test_gpu_gru.py's saturated gates)."""
    import torch
    from bsarec_amd.gru4rec import cand_scores_loss
    s, E, pos, neg = _head_inputs(33, 64, 301, 50.0)
    rl, _, rds, rdEc = R.head(s.numpy(), E.numpy(), pos.numpy(), neg.numpy(), loss, negatives, BPREG)
    gl, ds, dEc = _head_gpu(s, E, pos, neg, loss, negatives)
    assert np.isfinite(gl) and np.isfinite(ds).all() and np.isfinite(dEc).all()
    cand = torch.from_numpy(R.candidates(pos.numpy(), neg.numpy(), negatives))
    st, Ec = s.clone().requires_grad_(True), E[cand].clone().requires_grad_(True)
    tl = cand_scores_loss(st @ Ec.T, cand, pos, loss, BPREG)
    tl.backward()
    ours = (abs(gl - rl) / abs(rl), rel_l2(ds, rds), rel_l2(dEc, rdEc))
    theirs = (abs(tl.item() - rl) / abs(rl), rel_l2(st.grad.numpy(), rds), rel_l2(Ec.grad.numpy(), rdEc))
    print(f"cand head saturated {loss} {negatives}: loss {gl:.6f} (reference {rl:.6f}); loss / ds / dEc errors "
          f"HIP {ours[0]:.2e} {ours[1]:.2e} {ours[2]:.2e}  torch fp32 {theirs[0]:.2e} {theirs[1]:.2e} {theirs[2]:.2e}")
    for name, a, b in zip(("loss", "ds", "dEc"), ours, theirs):
        assert a <= 8.0 * b, (name, a, b)


# ---- the whole step ---------------------------------------------------------------------------------------------------------
def _step():
    import test_gpu_gru4rec_step as T
    return T


def _model(shape, p, loss, negatives, **kw):
    return _step()._model(shape, p, gru_loss=loss, gru_negatives=negatives, gru_bpreg=BPREG, **kw)


@functools.lru_cache(maxsize=None)
def _reference(shape, p, seed, step, loss, negatives):
    T = _step()
    V, d, H, N, L, B = T.SHAPES[shape]
    ids, pos, neg = (t.numpy() for t in T._batch(shape))
    mult = S.dropout_mult(B, L, d, p, seed, step)
    return R.loss_and_grads(T._params(T._model(shape)), ids, pos, neg, H, N, loss, negatives, BPREG, mult)


@pytest.mark.parametrize("loss,negatives", COMBOS)
@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("shape", [1, 2])
def test_loss_and_grads_against_the_reference(shape, p, loss, negatives):
    import torch
    T = _step()
    V, d, H, N, L, B = T.SHAPES[shape]
    m = _model(shape, p, loss, negatives)
    ids, pos, neg = (t.cuda() for t in T._batch(shape))
    val, grads = m.loss_and_grads(ids, pos, neg, train=True)
    st = m.step_state.cpu().tolist()                          # the seed and the counter of the mask, read back from the device
    assert st[1] == 1 and st[2] == 0
    rloss, rgrads = _reference(shape, p, st[0], st[1], loss, negatives)
    assert list(grads) == list(m.state_dict()) == S.keys(N)
    e_loss = abs(val.item() - rloss) / abs(rloss)
    errs = {k: rel_l2(g.cpu().numpy(), rgrads[k]) for k, g in grads.items()}
    g = grads["item_embeddings.weight"].cpu().numpy()
    assert np.isfinite(g).all()
    both = np.array([ids[6, -1].item(), ids[7, -1].item()])   # pos[6] and neg[7] of the batch
    e_both = rel_l2(g[both], rgrads["item_embeddings.weight"][both])
    print(f"cand step {loss} {negatives} shape {shape} p={p}: loss {val.item():.7f} rel {e_loss:.2e} rows(lookup+head) "
          f"{e_both:.2e} " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert e_loss <= LOSS_GATE
    for k, v in errs.items():
        assert v <= GRAD_GATE, (k, v)
    assert e_both <= GRAD_GATE
    used = [ids.reshape(-1), pos] + ([neg] if negatives != "in_batch" else [])
    rest = np.setdiff1d(np.arange(V), torch.unique(torch.cat(used)).cpu().numpy())
    assert not g[rest].any()                                  # exactly zero, every float written
    assert not rgrads["item_embeddings.weight"][rest].any()


@pytest.mark.parametrize("loss,negatives", COMBOS)
def test_three_train_steps_against_the_reference(loss, negatives):
    T = _step()
    V, d, H, N, L, B = T.SHAPES[1]
    p, wd = 0.5, 0.01
    m = _model(1, p, loss, negatives, weight_decay=wd, gru_step_graph=False)
    params = T._params(m)
    ids, pos, neg = T._batch(1)
    st = S.adam_state(lr=1e-3, weight_decay=wd)
    losses = []
    for step in range(1, 4):
        losses.append(m.train_step(ids.cuda(), pos.cuda(), neg.cuda()).item())
        rl = R.train_step(params, st, ids.numpy(), pos.numpy(), neg.numpy(), H, N, loss, negatives, BPREG,
                          S.dropout_mult(B, L, d, p, SEED, step))
        print(f"cand adam {loss} {negatives} step {step}: loss {losses[-1]:.7f} reference {rl:.7f}")
    assert np.isfinite(losses).all()
    state = m.step_state.cpu().tolist()
    assert state[0] == SEED and state[1] == 3 and state[2] == 3
    for k, q in m.named_parameters():
        e = rel_l2(q.detach().cpu().numpy(), params[k])
        print(f"cand adam x3 {loss} {negatives} {k}: {e:.2e}")
        assert e <= GRAD_GATE, (k, e)


def _three_steps(m, poison=False):
    import torch
    T = _step()
    V, d, H, N, L, B = T.SHAPES[1]
    ids, pos, neg = (t.cuda() for t in T._batch(1))
    losses = []
    for _ in range(3):
        if poison:
            m._slot(m._step_buffers(), B, L)["ws"].fill_(0xFF)      # NaN in every float, all ones in the accumulator
        losses.append(m.train_step(ids, pos, neg).clone())
    return torch.stack(losses), {k: v.detach().clone() for k, v in m.state_dict().items()}


@pytest.mark.parametrize("loss,negatives", COMBOS)
def test_determinism_with_a_poisoned_workspace(loss, negatives):
    import torch
    la, pa = _three_steps(_model(1, 0.5, loss, negatives, gru_step_graph=False))
    lb, pb = _three_steps(_model(1, 0.5, loss, negatives, gru_step_graph=False), poison=True)
    assert torch.isfinite(la).all() and torch.equal(la, lb)
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k


@pytest.mark.parametrize("loss,negatives", COMBOS)
def test_graph_replay_is_the_next_step(loss, negatives):
    import torch
    mg = _model(1, 0.5, loss, negatives)
    lg, pg = _three_steps(mg)
    le, pe = _three_steps(_model(1, 0.5, loss, negatives, gru_step_graph=False))
    assert mg._fused["slots"][(33, 20)]["graph"] is not None
    assert torch.equal(lg, le) and len(set(lg.tolist())) == 3
    for k in pg:
        assert torch.equal(pg[k], pe[k]), k
    assert mg.step_state.cpu().tolist()[1:3] == [3, 3]


@pytest.mark.parametrize("loss,negatives", COMBOS)
def test_torch_path_matches_the_fused_step(loss, negatives):
    """gru_step = "torch": calculate_loss + backward against the fused loss_and_grads at p = 0, at the gates."""
    T = _step()
    fused = _model(1, 0.0, loss, negatives)
    plain = _model(1, 0.0, loss, negatives, gru_step="torch")
    ids, pos, neg = (t.cuda() for t in T._batch(1))
    val, grads = fused.loss_and_grads(ids, pos, neg, train=False)
    tl = plain.calculate_loss(ids, pos, neg)
    tl.backward()
    e_loss = abs(tl.item() - val.item()) / abs(val.item())
    errs = {k: rel_l2(q.grad.cpu().numpy(), grads[k].cpu().numpy()) for k, q in plain.named_parameters()}
    print(f"cand torch path {loss} {negatives}: loss {tl.item():.7f} / {val.item():.7f} rel {e_loss:.2e} " +
          " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert list(errs) == list(grads)
    assert e_loss <= LOSS_GATE
    for k, v in errs.items():
        assert v <= GRAD_GATE, (k, v)


def test_main_run_with_bpr_max_and_the_checkpoint_round_trip(monkeypatch, tmp_path):
    import torch
    from bsarec_amd import data as Dm, main as M
    from test_gpu_gru4rec import _setup

    def no_optimiser(*a, **kw):
        raise AssertionError("a torch optimiser was built for a fused GRU4Rec")
    monkeypatch.setattr(torch.optim, "Adam", no_optimiser)
    msgs = []

    class Grab(logging.Handler):
        def emit(self, rec):
            msgs.append(rec.msg)
    logger = logging.getLogger("gru4rec_cand_main")
    logger.setLevel(logging.INFO)
    logger.propagate = False
    logger.addHandler(Grab())
    flags = ["--gru_step", "fused", "--gru_loss", "bpr_max", "--gru_negatives", "in_batch+sampled"]
    seqs = Dm.synth_ml1m_like(seed=5, n_users=200, n_items=300)
    args = M.parse_args(["--model_type", "GRU4Rec", "--gru_hidden_size", "64", "--max_seq_length", "20", "--batch_size", "256",
                         "--epochs", "2", "--patience", "100"] + flags)
    scores, info, epochs, secs = M.run(args, seqs, logger)
    losses = [float(ast.literal_eval(m)["rec_loss"]) for m in msgs if isinstance(m, str) and "'rec_loss'" in m]
    print(f"cand main.run bpr_max in_batch+sampled: losses {losses} scores {scores}")
    assert epochs == 2 and len(losses) == 2 and np.isfinite(losses).all()
    assert losses[1] < losses[0]
    assert len(scores) == 6 and np.isfinite(scores).all() and all(0.0 <= s <= 1.0 for s in scores)
    # the checkpoint round trip, bit for bit
    seqs, args, model, tr = _setup(flags)
    assert model.gru_step == "fused" and model.torch_optim is False and model._head.loss == 3 and model._head.candidates == 2
    tr.train(0)
    assert getattr(tr, "_torch_opt", None) is None and model.step_state[2].item() > 0
    path = str(tmp_path / "gru4rec_cand.pt")
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    tr.save(path)
    with torch.no_grad():
        for q in model.parameters():
            q.add_(1.0)
    tr.load(path)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
