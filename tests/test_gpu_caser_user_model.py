"""The personalised CaserModel (args.caser_user) on the GPU: torch mode against the twin module in double on the CPU (loss and every
parameter gradient at the gates of test_gpu_caser_model), main.run end to end in both step modes, the Trainer's evaluation passing
``user_ids``, the checkpoint round trip, and the flag-off model called through the Trainer's helper exactly as before.
(B, L, d) = (9, 12, 32), V = 50, U = 6, n_h = 16, n_v = 4."""
import argparse
import ast
import logging

import numpy as np
import pytest

from conftest import rel_l2
import caser_user_ref as UR

pytestmark = pytest.mark.gpu
OUT_GATE, GRAD_GATE, LOSS_GATE = 2e-5, 2e-4, 5e-6
V, U, D, L, B, NH, NV = 50, 6, 32, 12, 9, 16, 4
MODEL_SEED = 3            # the first seed from 0 at which the reference's condition holds (caser_user_ref.condition at 1e-4)


def _args(**kw):
    a = argparse.Namespace(item_size=V, num_users=U, hidden_size=D, max_seq_length=L, hidden_dropout_prob=0.0,
                           initializer_range=0.02, caser_nh=NH, caser_nv=NV, lr=1e-3, adam_beta1=0.9, adam_beta2=0.999,
                           weight_decay=0.0, caser_user=True)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _batch():
    import torch
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(1, V, (B, L), generator=g)
    ids[0, :7] = 0                                            # padding in front, not masked by this model
    ids[1, :11] = 0
    pos = torch.randint(1, V, (B,), generator=g)
    neg = torch.randint(1, V, (B,), generator=g)
    pos[0], neg[1] = ids[0, -1], ids[1, -1]                   # rows of the table that the lookup and the head both touch
    users = torch.tensor([0, 5, 2, 2, 5, 0, 3, 2, 1])         # 0, U - 1, repeats; user 4 is named by no row
    return ids, users, pos, neg


def _host_model(seed=MODEL_SEED, **kw):
    """Trained-size weights, as test_gpu_caser_model._model scales them, the user half alike."""
    import torch
    from bsarec_amd import CaserModel
    torch.manual_seed(seed)
    m = CaserModel(_args(**kw))
    with torch.no_grad():
        m.item_embeddings.weight.mul_(40.0)
        m.user_embeddings.weight.mul_(40.0)
        m.fc1.weight.mul_(5.0)
        m.fc1.bias.normal_(0.0, 0.1)
        m.fc2.weight.mul_(5.0)
        m.fc2.bias.normal_(0.0, 0.1)
    return m


def test_torch_mode_against_the_twin_in_double():
    import torch
    from test_caser_user_cpu import TwinUser
    m = _host_model()
    assert m.caser_step == "torch" and m.torch_optim is True and m.needs_user_ids is True
    state = {k: v.detach().clone() for k, v in m.state_dict().items()}
    ids, users, pos, neg = _batch()
    cells, umin = UR.condition({k: v.numpy().astype(np.float64) for k, v in state.items()}, ids.numpy(), users.numpy(), None, 1e-4)
    assert cells == 0 and umin >= 1e-4, (cells, umin)         # a condition on the inputs: no choice at fp32's rounding level
    twin = TwinUser(V, U, L, D, NH, NV).double()
    twin.load_state_dict({k: v.double() for k, v in state.items()})
    tl = twin.loss(ids, users, pos, neg)
    tl.backward()
    s_t = twin.state(ids, users).detach().numpy()
    m = m.cuda()
    m.train()
    loss = m.calculate_loss(ids.cuda(), pos.cuda(), neg.cuda(), user_ids=users.cuda())
    loss.backward()
    e_loss = abs(loss.item() - tl.item()) / abs(tl.item())
    errs = {}
    for (k, q), (k2, t) in zip(m.named_parameters(), twin.named_parameters()):
        assert k == k2
        ref, got = t.grad.numpy(), q.grad.cpu().numpy()
        if not ref.any():
            assert not got.any(), k
            continue
        errs[k] = rel_l2(got.reshape(ref.shape), ref)
    m.eval()
    with torch.no_grad():
        s = m(ids.cuda(), users.cuda())
        assert torch.equal(m.predict(ids.cuda(), users.view(B, 1).cuda()), s)
        assert torch.equal(m.last_hidden(ids.cuda(), users.cuda()), s)
    e_s = rel_l2(s.cpu().numpy(), s_t)
    worst = max((v, k) for k, v in errs.items())
    print(f"caser user model: loss {loss.item():.7f} rel {e_loss:.2e} s {e_s:.2e} alive {(s_t > 0).mean():.2f} "
          f"P {errs['user_embeddings.weight']:.2e} fc2 {errs['fc2.weight']:.2e} / {errs['fc2.bias']:.2e} worst {worst[0]:.2e} ({worst[1]})")
    assert e_loss <= LOSS_GATE and e_s <= OUT_GATE and (s_t > 0).mean() > 0.2
    for k, v in errs.items():
        assert v <= GRAD_GATE, (k, v)
    gP = m.user_embeddings.weight.grad.cpu().numpy()
    assert not gP[4].any() and gP[2].any()                    # a user no row names: exactly zero
    with pytest.raises(ValueError, match="needs user_ids"):
        m(ids.cuda())
    with pytest.raises(ValueError, match="user_ids must be"):
        m(ids.cuda(), users[:-1].cuda())


def _run(argv):
    import torch  # noqa: F401
    from bsarec_amd import data as Dm, main as M
    msgs = []

    class Grab(logging.Handler):
        def emit(self, rec):
            msgs.append(rec.msg)
    logger = logging.getLogger("caser_user_main")
    logger.setLevel(logging.INFO)
    logger.propagate = False
    logger.handlers = [Grab()]
    seqs = Dm.synth_ml1m_like(seed=5, n_users=120, n_items=200)
    args = M.parse_args(["--model_type", "Caser", "--caser_user", "--max_seq_length", "12", "--hidden_size", "32",
                         "--batch_size", "64", "--epochs", "2", "--patience", "100"] + argv)
    scores, info, epochs, secs = M.run(args, seqs, logger)
    losses = [float(ast.literal_eval(m)["rec_loss"]) for m in msgs if isinstance(m, str) and "'rec_loss'" in m]
    assert args.num_users == len(seqs) + 1
    return scores, losses, epochs


def test_main_run_with_the_fused_step(monkeypatch):
    import torch

    def no_optimiser(*a, **kw):
        raise AssertionError("a torch optimiser was built for a fused Caser")
    monkeypatch.setattr(torch.optim, "Adam", no_optimiser)
    scores, losses, epochs = _run(["--caser_step", "fused"])
    print(f"fused caser_user main.run: losses {losses} scores {scores}")
    assert epochs == 2 and len(losses) == 2 and np.isfinite(losses).all()
    assert losses[1] < losses[0]
    assert len(scores) == 6 and np.isfinite(scores).all() and all(0.0 <= s <= 1.0 for s in scores)


def test_main_run_in_torch_mode():
    scores, losses, epochs = _run(["--caser_step", "torch"])
    print(f"torch caser_user main.run: losses {losses} scores {scores}")
    assert epochs == 2 and len(losses) == 2 and np.isfinite(losses).all()
    assert losses[1] < losses[0]
    assert len(scores) == 6 and np.isfinite(scores).all() and all(0.0 <= s <= 1.0 for s in scores)


def _setup(argv):
    """What main.run builds before its epoch loop (test_gpu_caser_model._setup, with num_users as main.run sets it)."""
    import scipy.sparse as sp
    import torch
    from bsarec_amd import data as Dm, main as M
    from bsarec_amd.trainer import Trainer
    seqs = Dm.synth_ml1m_like(seed=5, n_users=120, n_items=200)
    args = M.parse_args(["--model_type", "Caser", "--max_seq_length", str(L), "--hidden_size", str(D), "--batch_size", "64",
                         "--epochs", "1", "--patience", "100"] + argv)
    args.item_size = max(max(s) for s in seqs) + 1
    args.num_users = len(seqs) + 1
    dev = torch.device("cuda", torch.cuda.current_device())
    u, x, a = Dm.train_table(seqs, L)
    train_dl = Dm.DeviceBatches(u, x, a, args.batch_size, dev, shuffle=True, seed=args.seed)
    eval_dl = Dm.DeviceBatches(*Dm.eval_table(seqs, L, "valid"), args.batch_size, dev, shuffle=False)
    test_dl = Dm.DeviceBatches(*Dm.eval_table(seqs, L, "test"), args.batch_size, dev, shuffle=False)
    for split in ("valid", "test"):
        indptr, cols = Dm.seen_csr(seqs, split)
        setattr(args, f"{split}_rating_matrix", sp.csr_matrix((np.ones(len(cols)), cols, indptr), shape=(len(seqs), args.item_size)))
    torch.manual_seed(args.seed)
    model = M.MODEL_DICT[args.model_type.lower()](args=args)
    train_dl.enable_negatives(seqs, args.item_size)
    model.set_seed(args.seed)
    return seqs, args, model, Trainer(model, train_dl, eval_dl, test_dl, args)


def _spy(model, name, calls):
    fn = getattr(model, name)

    def wrapped(*a, **kw):
        calls.append((name, len(a), dict(kw)))
        return fn(*a, **kw)
    setattr(model, name, wrapped)


def test_evaluation_and_training_pass_user_ids_and_the_checkpoint_round_trips(tmp_path):
    import torch
    seqs, args, model, tr = _setup(["--caser_user", "--caser_step", "fused"])
    assert model.needs_user_ids is True and model.user_embeddings.num_embeddings == len(seqs) + 1
    calls = []
    _spy(model, "last_hidden", calls)
    _spy(model, "train_step", calls)
    tr.train(0)
    assert getattr(tr, "_torch_opt", None) is None and model.step_state[2].item() > 0
    scores, _ = tr.test(0)                                    # topk_full
    args.eval_full_rank = "rank"
    tr.test(0)                                                # answer_ranks
    args.eval_negatives = 20
    tr.test(0)                                                # sampled_ranks
    del args.eval_negatives, args.eval_full_rank
    assert len(scores) == 6 and np.isfinite(scores).all()
    seen = {name for name, _, _ in calls}
    assert seen == {"last_hidden", "train_step"}
    n_eval = len([c for c in calls if c[0] == "last_hidden"])
    assert n_eval == 3 * len(list(tr.test_dataloader))        # every evaluation site went through the helper
    users_of = {}
    for name, n_pos, kw in calls:
        assert set(kw) == {"user_ids"} and kw["user_ids"] is not None, (name, kw)
        users_of.setdefault(name, []).append(kw["user_ids"])
    batch = next(iter(tr.test_dataloader))
    users, ids = batch[0], batch[1]
    assert torch.equal(users_of["last_hidden"][0], users)     # the batch's own user ids, in its order
    # the state depends on them: other users for the same sequences give another state
    model.eval()
    h = model.last_hidden(ids, users)
    assert torch.equal(h, model.last_hidden(ids, users.clone())) and not torch.equal(h, model.last_hidden(ids, users.roll(1)))
    # checkpoint: bit for bit, user table and fc2 included, and the step goes on in place
    path = str(tmp_path / "caser_user.pt")
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert "user_embeddings.weight" in before and "fc2.bias" in before
    tr.save(path)
    with torch.no_grad():
        for q in model.parameters():
            q.add_(1.0)
    tr.load(path)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
    t = model.step_state[2].item()
    tr.train(1)
    assert model.step_state[2].item() > t
    assert not torch.equal(model.state_dict()["user_embeddings.weight"], before["user_embeddings.weight"])
    assert not torch.equal(model.state_dict()["fc2.weight"], before["fc2.weight"])


def test_the_default_model_is_called_as_before():
    """Flag off: the Trainer's helper passes no user_ids, and what it returns has the bits of the direct call of the parent's
    call sites (train_step / last_hidden / loss_and_grads with the positional arguments alone)."""
    import torch
    seqs, args, model, tr = _setup(["--caser_step", "fused"])
    seqs2, args2, twin, tr2 = _setup(["--caser_step", "fused"])
    assert model.needs_user_ids is False and not hasattr(model, "user_embeddings")
    assert list(model.state_dict()) == list(twin.state_dict()) and "fc2.weight" not in model.state_dict()
    users, ids, ans, neg = next(iter(tr.train_dataloader))[:4]
    calls = []
    for name in ("loss_and_grads", "train_step", "last_hidden"):
        _spy(model, name, calls)
    loss_h, grads_h = tr._with_users(model.loss_and_grads, users, ids, ans, neg)
    loss_d, grads_d = twin.loss_and_grads(ids, ans, neg)
    assert torch.equal(loss_h, loss_d) and list(grads_h) == list(grads_d)
    for k in grads_h:
        assert torch.equal(grads_h[k], grads_d[k]), k
    step_h = tr._with_users(model.train_step, users, ids, ans, neg).clone()
    step_d = twin.train_step(ids, ans, neg).clone()
    assert torch.equal(step_h, step_d)
    for k, v in model.state_dict().items():
        assert torch.equal(v, twin.state_dict()[k]), k
    assert torch.equal(tr._with_users(model.last_hidden, users, ids), twin.last_hidden(ids))
    tr.train(0)
    tr.test(0)
    assert calls and all(kw == {} for _, _, kw in calls), calls          # never a user_ids keyword
