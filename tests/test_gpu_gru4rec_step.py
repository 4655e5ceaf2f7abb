"""The fused GRU4Rec step on the GPU (gru_step = "fused": bsarec_gru4rec_loss_grad / bsarec_gru4rec_train_step) against the step in
numpy double (gru4rec_step_ref): loss and every gradient at p = 0 and p = 0.5 on three shapes, three Adam steps, bit determinism
with a poisoned workspace, graph replay against eager calls, and the trainer end to end.

  shape 1  V = 301, d = 64, H = 64, N = 2, L = 20, B = 33   660 tokens: no multiple of the scatter chunk; B one past two 16-row tiles
  shape 2  V = 5, d = 36, H = 32, N = 1, L = 1, B = 17      d no multiple of 32, L = 1, every row of the table hit many times
  shape 3  V = 40, d = 256, H = 128, N = 1, L = 3, B = 65   the widest rows (64 float4 lanes per row)"""
import argparse
import ast
import functools
import logging

import numpy as np
import pytest

from conftest import rel_l2
import gru4rec_step_ref as S

pytestmark = pytest.mark.gpu
LOSS_GATE, GRAD_GATE = 5e-6, 2e-4
SHAPES = {1: (301, 64, 64, 2, 20, 33), 2: (5, 36, 32, 1, 1, 17), 3: (40, 256, 128, 1, 3, 65)}
SEED = 5


def _args(shape, p=0.0, **kw):
    V, d, H, N, L, B = SHAPES[shape]
    a = argparse.Namespace(item_size=V, hidden_size=d, gru_hidden_size=H, num_hidden_layers=N, max_seq_length=L,
                           hidden_dropout_prob=p, initializer_range=0.02, lr=1e-3, adam_beta1=0.9, adam_beta2=0.999,
                           weight_decay=0.0, gru_step="fused")
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@functools.lru_cache(maxsize=None)
def _batch(shape):
    """As test_gpu_gru4rec._batch, with the collisions of the item-table gradient: padding zeros in front, an answer and a negative
    equal to a looked-up id, a row whose answer is its negative, a negative equal to another row's answer."""
    import torch
    V, d, H, N, L, B = SHAPES[shape]
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(1, V, (B, L), generator=g)
    ids[:5, :max(1, min(7, L - 1))] = 0
    pos = torch.randint(1, V, (B,), generator=g)
    neg = torch.randint(1, V, (B,), generator=g)
    pos[6], neg[7] = ids[6, -1], ids[7, -1]
    neg[8] = pos[8]
    neg[9] = pos[10]
    return ids, pos, neg


def _model(shape, p=0.0, **kw):
    """A fused-step model on the GPU with trained-size weights (as test_gpu_gru4rec._pair: the gates leave the linear range); the
    same weights for every p and option."""
    import torch
    from bsarec_amd import GRU4RecModel
    torch.manual_seed(7 + shape)
    m = GRU4RecModel(_args(shape, p, **kw))
    with torch.no_grad():
        m.item_embeddings.weight.mul_(25.0)
        m.dense.weight.mul_(10.0)
        m.dense.bias.normal_(0.0, 0.1)
    m = m.cuda()
    m.train()
    m.set_seed(SEED)
    return m


def _params(m):
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in m.state_dict().items()}


@functools.lru_cache(maxsize=None)
def _reference(shape, p, seed, step):
    """Loss and gradients of the reference at the model's initial weights, under the mask of (seed, step): computed once."""
    V, d, H, N, L, B = SHAPES[shape]
    ids, pos, neg = (t.numpy() for t in _batch(shape))
    mult = S.dropout_mult(B, L, d, p, seed, step)
    return S.loss_and_grads(_params(_model(shape)), ids, pos, neg, H, N, mult)


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("shape", [1, 2, 3])
def test_loss_and_grads_against_the_reference(shape, p):
    import torch
    V, d, H, N, L, B = SHAPES[shape]
    m = _model(shape, p)
    ids, pos, neg = (t.cuda() for t in _batch(shape))
    loss, grads = m.loss_and_grads(ids, pos, neg, train=True)
    st = m.step_state.cpu().tolist()
    assert st[1] == 1 and st[2] == 0                          # the step counter advanced once, Adam's t did not
    rloss, rgrads = _reference(shape, p, st[0], st[1])
    assert list(grads) == list(m.state_dict()) == S.keys(N)
    e_loss = abs(loss.item() - rloss) / abs(rloss)
    errs = {k: rel_l2(g.cpu().numpy(), rgrads[k]) for k, g in grads.items()}
    g = grads["item_embeddings.weight"].cpu().numpy()
    both = np.array([ids[6, -1].item(), ids[7, -1].item()])
    e_both = rel_l2(g[both], rgrads["item_embeddings.weight"][both])
    print(f"gru4rec step shape {shape} p={p}: loss {loss.item():.7f} rel {e_loss:.2e} rows(lookup+head) {e_both:.2e} " +
          " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert e_loss <= LOSS_GATE
    for k, v in errs.items():
        assert v <= GRAD_GATE, (k, v)
    assert e_both <= GRAD_GATE
    touched = torch.unique(torch.cat([ids.reshape(-1), pos, neg])).cpu().numpy()
    rest = np.setdiff1d(np.arange(V), touched)
    assert not g[rest].any()                                  # exactly zero, every float written
    assert not rgrads["item_embeddings.weight"][rest].any()
    # the same call again: the next mask at p > 0, the same bits at p = 0
    loss2, grads2 = m.loss_and_grads(ids, pos, neg, train=True)
    assert m.step_state[1].item() == 2
    same = all(torch.equal(grads[k], grads2[k]) for k in grads) and torch.equal(loss, loss2)
    assert same == (p == 0.0)
    if p > 0.0:
        # train = 0 draws nothing and touches no counter: the bits of the p = 0 model
        loss0, grads0 = m.loss_and_grads(ids, pos, neg, train=False)
        assert m.step_state[1].item() == 2
        lossz, gradsz = _model(shape, 0.0).loss_and_grads(ids, pos, neg, train=True)
        assert torch.equal(loss0, lossz)
        for k in grads0:
            assert torch.equal(grads0[k], gradsz[k]), k


def test_a_row_whose_answer_is_its_negative_adds_exactly_nothing():
    """Row 8 of the batch has answers == neg_answers: diff = 0 exactly, and its two head rows cancel in the fixed-point sum.  With
    that sequence's tokens and head taken out of the reference, the item-table gradient of the id is still met -- and an id that
    ONLY that head touches stays exactly zero."""
    import torch
    V, d, H, N, L, B = SHAPES[1]
    m = _model(1)
    ids, pos, neg = (t.clone() for t in _batch(1))
    lone = int(np.setdiff1d(np.arange(1, V), torch.cat([ids.reshape(-1), pos, neg]).numpy())[0])
    pos[8] = neg[8] = lone
    _, grads = m.loss_and_grads(ids.cuda(), pos.cuda(), neg.cuda(), train=False)
    assert not grads["item_embeddings.weight"][lone].any().item()


@pytest.mark.parametrize("p,wd", [(0.0, 0.0), (0.5, 0.0), (0.5, 0.01)])
def test_three_train_steps_against_the_reference(p, wd):
    import torch
    V, d, H, N, L, B = SHAPES[1]
    m = _model(1, p, weight_decay=wd, gru_step_graph=False)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    params = _params(m)
    ids, pos, neg = _batch(1)
    st = S.adam_state(lr=1e-3, weight_decay=wd)
    losses = []
    for step in range(1, 4):
        losses.append(m.train_step(ids.cuda(), pos.cuda(), neg.cuda()).item())
        rl = S.train_step(params, st, ids.numpy(), pos.numpy(), neg.numpy(), H, N, S.dropout_mult(B, L, d, p, SEED, step))
        print(f"fused adam p={p} wd={wd} step {step}: loss {losses[-1]:.7f} reference {rl:.7f}")
    assert np.isfinite(losses).all()
    state = m.step_state.cpu().tolist()
    assert state[0] == SEED and state[1] == 3 and state[2] == 3
    flat = m.gru_layers._flat
    off = 0
    for k, q in m.named_parameters():
        e = rel_l2(q.detach().cpu().numpy(), params[k])
        print(f"fused adam x3 p={p} wd={wd} {k}: {e:.2e}")
        assert e <= 2e-4, (k, e)
        assert not torch.equal(q.detach(), before[k])                                 # it moved
        if k != "item_embeddings.weight":                       # updated in place: still views of the flat array
            assert q.data_ptr() == flat.data_ptr() + 4 * off, k
            off += q.numel()
    assert off == flat.numel()


def _three_steps(m, poison=False):
    import torch
    V, d, H, N, L, B = SHAPES[1]
    ids, pos, neg = (t.cuda() for t in _batch(1))
    losses = []
    for _ in range(3):
        if poison:
            m._slot(m._step_buffers(), B, L)["ws"].fill_(0xFF)      # NaN in every float, all ones in the accumulator
        losses.append(m.train_step(ids, pos, neg).clone())
    return torch.stack(losses), {k: v.detach().clone() for k, v in m.state_dict().items()}


def test_determinism_with_a_poisoned_workspace():
    import torch
    la, pa = _three_steps(_model(1, 0.5, gru_step_graph=False))
    lb, pb = _three_steps(_model(1, 0.5, gru_step_graph=False), poison=True)
    assert torch.isfinite(la).all() and torch.equal(la, lb)
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k


def test_graph_replay_is_the_next_step():
    import torch
    mg = _model(1, 0.5)
    lg, pg = _three_steps(mg)
    le, pe = _three_steps(_model(1, 0.5, gru_step_graph=False))
    assert mg._fused["slots"][(33, 20)]["graph"] is not None
    assert torch.equal(lg, le) and len(set(lg.tolist())) == 3      # three different masks, three different t
    for k in pg:
        assert torch.equal(pg[k], pe[k]), k
    assert mg.step_state.cpu().tolist()[1:3] == [3, 3]


def test_main_run_with_the_fused_step(monkeypatch):
    import torch
    from bsarec_amd import data as Dm, main as M

    def no_optimiser(*a, **kw):
        raise AssertionError("a torch optimiser was built for a fused GRU4Rec")
    monkeypatch.setattr(torch.optim, "Adam", no_optimiser)
    msgs = []

    class Grab(logging.Handler):
        def emit(self, rec):
            msgs.append(rec.msg)
    logger = logging.getLogger("gru4rec_step_main")
    logger.setLevel(logging.INFO)
    logger.propagate = False
    logger.addHandler(Grab())
    seqs = Dm.synth_ml1m_like(seed=5, n_users=200, n_items=300)
    args = M.parse_args(["--model_type", "GRU4Rec", "--gru_step", "fused", "--gru_hidden_size", "64", "--max_seq_length", "20",
                         "--batch_size", "256", "--epochs", "2", "--patience", "100"])
    scores, info, epochs, secs = M.run(args, seqs, logger)
    losses = [float(ast.literal_eval(m)["rec_loss"]) for m in msgs if isinstance(m, str) and "'rec_loss'" in m]
    print(f"fused main.run: losses {losses} scores {scores}")
    assert epochs == 2 and len(losses) == 2 and np.isfinite(losses).all()
    assert losses[1] < losses[0]
    assert len(scores) == 6 and np.isfinite(scores).all() and all(0.0 <= s <= 1.0 for s in scores)


def test_trainer_mode_switch_and_checkpoint_round_trip(tmp_path):
    import torch
    from bsarec_amd import GRU4RecModel
    from test_gpu_gru4rec import _setup
    with pytest.raises(ValueError, match="gru_step"):
        GRU4RecModel(_args(1, gru_step="bogus"))
    default = GRU4RecModel(_args(1, gru_step="torch")).cuda()
    ids, pos, neg = (t.cuda() for t in _batch(1))
    with pytest.raises(RuntimeError, match="torch.optim.Adam"):
        default.train_step(ids, pos, neg)
    seqs, args, model, tr = _setup(["--gru_step", "fused"])
    assert model.gru_step == "fused" and model.torch_optim is False
    tr.train(0)
    assert getattr(tr, "_torch_opt", None) is None
    assert model.step_state[2].item() > 0                     # Adam's t: the steps ran in the library
    path = str(tmp_path / "gru4rec_fused.pt")
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    tr.save(path)
    with torch.no_grad():
        for q in model.parameters():
            q.add_(1.0)
    tr.load(path)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
    t = model.step_state[2].item()
    tr.train(1)                                               # the step still updates the loaded arrays in place
    assert model.step_state[2].item() > t
    assert any(not torch.equal(v, before[k]) for k, v in model.state_dict().items())
