"""The fused Mamba4Rec step on the GPU (mamba_step = "fused": bsarec_mamba4rec_loss_grad / bsarec_mamba4rec_train_step) against
the step in numpy double (mamba4rec_step_ref): loss and every gradient at p = 0 and at p = 0.5 under the masks of the device state
on four shapes, the eval-mode loss against calculate_loss, three Adam steps, bit determinism with a poisoned workspace, graph
replay against eager calls, and the trainer end to end.

  shape 1  V = 301, d = 64, N = 2, L = 20, B = 33; E = 2, d_state = 16, K = 4, R = 4    two state checkpoints (every 8th step),
                                                                                     660 tokens, the layer's defaults at d = 64
  shape 2  V = 5, d = 4, N = 1, L = 1, B = 17; E = 1, d_state = 4, K = 2, R = 4         L = 1, no checkpoint, the smallest d; V < B:
                                                                                     ids and answers collide; dA_log exactly 0
  shape 3  V = 40, d = 256, N = 1, L = 3, B = 65; E = 2, d_state = 32, K = 4, R = 16    d_inner = 512, d_state = 32, L < K, B one past
                                                                                     a 64-row tile
  shape 4  V = 23, d = 100, N = 2, L = 17, B = 5; E = 2, d_state = 16, K = 3, R = 8     d no power of two, L one past a checkpoint
                                                                                     edge, K = 3

Gates: those of test_gpu_lrurec_step.py and test_gpu_mamba4rec.py -- the loss to 5e-6 relative, every gradient tensor <= 2e-4
rel-L2, the parameters after three Adam steps <= 2e-4 rel-L2."""
import argparse
import ast
import functools
import logging

import numpy as np
import pytest

from conftest import rel_l2
import mamba_ref as R
import mamba4rec_step_ref as S

pytestmark = pytest.mark.gpu
LOSS_GATE, GRAD_GATE = 5e-6, 2e-4
SHAPES = {1: (301, 64, 2, 20, 33), 2: (5, 4, 1, 1, 17), 3: (40, 256, 1, 3, 65), 4: (23, 100, 2, 17, 5)}      # V, d, N, L, B
HYPER = {1: (2, 16, 4, 4), 2: (1, 4, 2, 4), 3: (2, 32, 4, 16), 4: (2, 16, 3, 8)}          # expand, d_state, d_conv, dt_rank
SEED = 5


def _args(shape, p=0.0, **kw):
    V, d, N, L, B = SHAPES[shape]
    E, ds, K, Rk = HYPER[shape]
    a = argparse.Namespace(item_size=V, hidden_size=d, num_hidden_layers=N, max_seq_length=L, hidden_dropout_prob=p,
                           initializer_range=0.1, lr=1e-3, adam_beta1=0.9, adam_beta2=0.999, weight_decay=0.0,
                           mamba_expand=E, mamba_d_state=ds, mamba_d_conv=K, mamba_dt_rank=Rk, mamba_step="fused")
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@functools.lru_cache(maxsize=None)
def _batch(shape):
    """Left-padded ids with a full row, a row of padding alone and a row whose first item is at L - 1; answers of which some are
    looked-up ids (of their own row and of another), so that the lookup and the head's answer term meet on a row of dE.  The
    asserts are conditions on the inputs (the seeds were chosen on the CPU so that they hold)."""
    V, d, N, L, B = SHAPES[shape]
    rng = np.random.default_rng(10 + shape)
    first = list(rng.integers(0, L, B))
    first[0], first[1], first[2] = 0, L, L - 1
    ids = R.ragged_ids(rng, B, L, first, V)
    ans = rng.integers(1, V, B)
    ans[0], ans[3] = ids[0, -1], ids[2, -1]
    assert ids[0].all() and not ids[1].any() and ids[2, -1] != 0 and not ids[2, :-1].any()
    assert len(np.intersect1d(np.unique(ids), np.unique(ans))) >= 2
    return ids, ans


def _model(shape, p=0.0, **kw):
    """A fused-step model on the GPU, LayerNorms and biases (but dt_proj's) off their init so that they matter (as
    test_gpu_mamba4rec._model); the same weights for every p and option."""
    import torch
    from bsarec_amd import Mamba4RecModel
    torch.manual_seed(7 + shape)
    m = Mamba4RecModel(_args(shape, p, **kw))
    with torch.no_grad():
        for k, q in m.named_parameters():
            if "LayerNorm" in k or (k.endswith(".bias") and "dt_proj" not in k):
                q.add_(0.1 * torch.randn_like(q))
    m = m.cuda()
    m.train()
    m.set_seed(SEED)
    return m


def _params(m):
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in m.state_dict().items()}


def _cuda(shape):
    import torch
    return tuple(torch.from_numpy(a).cuda() for a in _batch(shape))


@functools.lru_cache(maxsize=None)
def _reference(shape, p, seed, step):
    """Loss and gradients of the reference at the model's initial weights, under the masks of (seed, step): computed once."""
    V, d, N, L, B = SHAPES[shape]
    ids, ans = _batch(shape)
    loss, grads, _ = S.loss_and_grads(_params(_model(shape)), ids, ans, N, HYPER[shape],
                                      S.dropout_mults(B, L, d, N, p, seed, step))
    return loss, grads


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("shape", [1, 2, 3, 4])
def test_loss_and_grads_against_the_reference(shape, p):
    import torch
    V, d, N, L, B = SHAPES[shape]
    m = _model(shape, p)
    ids, ans = _cuda(shape)
    loss, grads = m.loss_and_grads(ids, ans, train=True)
    st = m.step_state.cpu().tolist()
    assert st[0] == SEED and st[1] == 1 and st[2] == 0        # the step counter advanced once, Adam's t did not
    rloss, rgrads = _reference(shape, p, st[0], st[1])        # the masks of the seed and counter READ BACK from the device
    assert sorted(grads) == sorted(m.state_dict()) and list(m.state_dict()) == S.keys(N, HYPER[shape], d)
    assert list(grads)[1:] == S.flat_keys(N, HYPER[shape], d)
    e_loss = abs(loss.item() - rloss) / abs(rloss)
    errs = {k: rel_l2(g.cpu().numpy(), rgrads[k]) for k, g in grads.items()}
    g = grads["item_embeddings.weight"].cpu().numpy()
    both = np.intersect1d(np.unique(_batch(shape)[0]), np.unique(_batch(shape)[1]))      # looked up AND some row's answer
    assert len(both) >= 2
    e_both = rel_l2(g[both], rgrads["item_embeddings.weight"][both])
    print(f"mamba4rec step shape {shape} p={p}: loss {loss.item():.7f} rel {e_loss:.2e} rows(lookup+head) {e_both:.2e} " +
          " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert e_loss <= LOSS_GATE
    for k, v in errs.items():
        assert v <= GRAD_GATE, (k, v)
    assert e_both <= GRAD_GATE
    if L == 1:                                                  # no earlier state: dA_log is exactly 0
        assert not grads["item_encoder.blocks.0.mamba.A_log"].any()
    # the same call again: the next masks at p > 0, the same bits at p = 0
    loss2, grads2 = m.loss_and_grads(ids, ans, train=True)
    assert m.step_state[1].item() == 2
    same = all(torch.equal(grads[k], grads2[k]) for k in grads) and torch.equal(loss, loss2)
    assert same == (p == 0.0)
    # train = 0 draws nothing and touches no counter: the bits of the p = 0 model, whatever p
    loss0, grads0 = m.loss_and_grads(ids, ans)
    assert m.step_state[1].item() == 2
    if p > 0.0:
        lossz, gradsz = _model(shape, 0.0).loss_and_grads(ids, ans, train=True)
        assert torch.equal(loss0, lossz)
        for k in grads0:
            assert torch.equal(grads0[k], gradsz[k]), k
    # ... and the loss of the model's own eval path, which evaluation ranks with
    m.eval()
    with torch.no_grad():
        want = m.calculate_loss(ids, ans).item()
    e_eval = abs(loss0.item() - want) / abs(want)
    print(f"mamba4rec step shape {shape} p={p}: loss(train=False) {loss0.item():.7f} calculate_loss(eval) {want:.7f} "
          f"rel {e_eval:.2e}")
    assert e_eval <= LOSS_GATE


@pytest.mark.parametrize("p,wd", [(0.0, 0.0), (0.5, 0.0), (0.5, 0.01)])
def test_three_train_steps_against_the_reference(p, wd):
    import torch
    V, d, N, L, B = SHAPES[1]
    m = _model(1, p, weight_decay=wd, mamba_step_graph=False)
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    params = _params(m)
    ids, ans = _batch(1)
    tid, tans = _cuda(1)
    st = S.adam_state(lr=1e-3, weight_decay=wd)
    losses = []
    for step in range(1, 4):
        losses.append(m.train_step(tid, tans).item())
        rl = S.train_step(params, st, ids, ans, N, HYPER[1], S.dropout_mults(B, L, d, N, p, SEED, step))
        print(f"fused adam p={p} wd={wd} step {step}: loss {losses[-1]:.7f} reference {rl:.7f}")
    assert np.isfinite(losses).all()
    state = m.step_state.cpu().tolist()
    assert state[0] == SEED and state[1] == 3 and state[2] == 3
    flat = m._wflat
    named = dict(m.named_parameters())
    for k, q in named.items():
        e = rel_l2(q.detach().cpu().numpy(), params[k])
        print(f"fused adam x3 p={p} wd={wd} {k}: {e:.2e}")
        assert e <= 2e-4, (k, e)
        assert not torch.equal(q.detach(), before[k])                                 # it moved
    off = 0
    for k in S.flat_keys(N, HYPER[1], d):                       # updated in place: still views of the flat array
        assert named[k].data_ptr() == flat.data_ptr() + 4 * off, k
        off += named[k].numel()
    assert off == flat.numel()
    for k, blk in enumerate(m.item_encoder.blocks):             # ... and each layer's array still a slice of it
        la = blk.mamba
        assert la._flat.data_ptr() == named[f"item_encoder.blocks.{k}.mamba.in_proj.weight"].data_ptr()
        assert all(q.data_ptr() == la._flat.data_ptr() + 4 * o for q, (o, n, s) in zip(la.flat_parameters(), la._slices.values()))


def _three_steps(m, poison=False):
    import torch
    V, d, N, L, B = SHAPES[1]
    ids, ans = _cuda(1)
    losses = []
    for _ in range(3):
        if poison:
            m._slot(m._step_buffers(), B, L)["ws"].fill_(0xFF)      # NaN in every float, all ones in the accumulator
        losses.append(m.train_step(ids, ans).clone())
    return torch.stack(losses), {k: v.detach().clone() for k, v in m.state_dict().items()}


def test_determinism_with_a_poisoned_workspace():
    import torch
    la, pa = _three_steps(_model(1, 0.5, mamba_step_graph=False))
    lb, pb = _three_steps(_model(1, 0.5, mamba_step_graph=False), poison=True)
    assert torch.isfinite(la).all() and torch.equal(la, lb)
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k


def test_graph_replay_is_the_next_step():
    import torch
    mg = _model(1, 0.5)
    lg, pg = _three_steps(mg)
    le, pe = _three_steps(_model(1, 0.5, mamba_step_graph=False))
    assert mg._fused["slots"][(33, 20)]["graph"] is not None
    assert torch.equal(lg, le) and len(set(lg.tolist())) == 3      # three different masks, three different t
    for k in pg:
        assert torch.equal(pg[k], pe[k]), k
    assert mg.step_state.cpu().tolist()[1:3] == [3, 3]


def test_main_run_with_the_fused_step(monkeypatch):
    import torch
    from bsarec_amd import data as Dm, main as M

    def no_optimiser(*a, **kw):
        raise AssertionError("a torch optimiser was built for a fused Mamba4Rec")
    monkeypatch.setattr(torch.optim, "Adam", no_optimiser)
    msgs = []

    class Grab(logging.Handler):
        def emit(self, rec):
            msgs.append(rec.msg)
    logger = logging.getLogger("mamba4rec_step_main")
    logger.setLevel(logging.INFO)
    logger.propagate = False
    logger.addHandler(Grab())
    seqs = Dm.synth_ml1m_like(seed=5, n_users=200, n_items=300)
    args = M.parse_args(["--model_type", "Mamba4Rec", "--mamba_step", "fused", "--max_seq_length", "20", "--batch_size", "256",
                         "--epochs", "2", "--patience", "100"])
    scores, info, epochs, secs = M.run(args, seqs, logger)
    losses = [float(ast.literal_eval(m)["rec_loss"]) for m in msgs if isinstance(m, str) and "'rec_loss'" in m]
    print(f"fused main.run: losses {losses} scores {scores}")
    assert epochs == 2 and len(losses) == 2 and np.isfinite(losses).all()
    assert losses[1] < losses[0]
    assert len(scores) == 6 and np.isfinite(scores).all() and all(0.0 <= s <= 1.0 for s in scores)


def test_trainer_evaluation_paths_and_checkpoint_round_trip(tmp_path):
    import torch
    from bsarec_amd import Mamba4RecModel
    from test_gpu_mamba4rec import _setup
    with pytest.raises(ValueError, match="mamba_step"):
        Mamba4RecModel(_args(1, mamba_step="bogus"))
    default = Mamba4RecModel(_args(1, mamba_step="torch")).cuda()
    ids, ans = _cuda(1)
    with pytest.raises(RuntimeError, match="torch.optim.Adam"):
        default.train_step(ids, ans)
    seqs, args, model, tr, test_dl = _setup(["--mamba_step", "fused"])
    model = tr.model
    assert model.mamba_step == "fused" and model.torch_optim is False and model.own_train_step is True
    first = float(tr.train(0)["rec_loss"])
    assert np.isfinite(first)
    assert getattr(tr, "_torch_opt", None) is None and not tr._graphs          # no torch optimiser, no capture by the Trainer
    t = model.step_state[2].item()
    assert t > 0 and model.step_state[1].item() == t           # Adam's t and the mask counter: the steps ran in the library
    assert any(s["graph"] is not None for s in model._fused["slots"].values())          # ... replayed from the model's own graph
    # the three evaluation paths agree as they do in the default mode
    dense, _ = tr.test(0)
    args.eval_full_rank = "fused"
    fused, _ = tr.test(0)
    args.eval_full_rank = "rank"
    rank, _ = tr.test(0)
    del args.eval_full_rank
    assert len(fused) == 6 and np.isfinite(fused).all() and len(rank) == 7
    assert list(dense) == list(fused) and np.allclose(rank[:6], fused, rtol=0, atol=1e-12)
    # checkpoint: bit for bit back into the flat array, and into a model of the default mode
    path = str(tmp_path / "mamba4rec_fused.pt")
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    tr.save(path)
    with torch.no_grad():
        for q in model.parameters():
            q.add_(1.0)
    tr.load(path)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
    args.mamba_step = "torch"
    other = Mamba4RecModel(args).cuda()
    other.load_state_dict(torch.load(path))
    for k, v in other.state_dict().items():
        assert torch.equal(v, before[k]), k
    other.eval()
    model.eval()
    some = next(iter(test_dl))[1]
    assert torch.equal(other.last_hidden(some), model.last_hidden(some))
    tr.train(1)                                               # the step still updates the loaded arrays in place
    assert model.step_state[2].item() > t
    assert any(not torch.equal(v, before[k]) for k, v in model.state_dict().items())
