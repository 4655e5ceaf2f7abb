"""What the GPU tests of the one-call training steps (test_gpu_*_step.py) have in common, as plain functions of a per-model
description: the two batch builders, the first call with its state assertions, the comparison with the reference, the second-call /
train = False / eval-path tail, the row whose answer is its negative, the three Adam steps, bit determinism with a poisoned
workspace, graph replay, main.run, and the two trainer round trips (the pairwise "mode switch" and the block "evaluation paths").

A file keeps its shape table, seeds and gates as literals, builds ONE description with ``describe`` and keeps every test function
under its own name as a short call into this module; what only that model has (flat-array layouts, Caser's condition on the
inputs, the user table) stays in the file.  Batches and references are computed once per (description, arguments).  torch is
imported inside the functions, so a file that uses this module still collects on a host without a GPU."""
import ast
import importlib
import logging
import types

import numpy as np
import pytest

from conftest import rel_l2

_DEFAULTS = dict(
    call=lambda batch: (tuple(batch), {}),    # the device batch -> (positional, keyword) arguments of loss_and_grads / train_step
    eval_kw={},                  # how train = False is asked for: {} where it is the default, dict(train=False) where it is not
    eval_loss=True,              # the train = False loss is compared with calculate_loss in eval mode (a string: why it cannot be)
    adam_tag="fused adam",       # the head of the lines of the three Adam steps
    moved=None,                  # None: every parameter must have moved, and each prints its line; a list: those must have
                                 # moved, and one line names the worst parameter
    before_step=None,            # before_step(params, host batch, mult, what): a condition on the inputs of each Adam step
    main=None,                   # main.run: dict(argv=..., synth=dict(n_users, n_items), tag=the head of its line)
    trainer=None)                # the trainer round trip: (the module that has _setup, a head weight that training moves)
_NEEDED = ("stem", "name", "flag", "seed", "loss_gate", "grad_gate", "vbl", "slot", "args", "model", "batch", "reference", "mults",
           "train_step")
MAIN = dict(argv=["--max_seq_length", "20", "--batch_size", "256"], synth=dict(n_users=200, n_items=300), tag="fused main.run")
_once = {}


def describe(**kw):
    """stem: file-name stem, cache key and (with "_" as " ", then " step") the head of the printed lines; name: ``--model_type``
    and, with "Model", the class; flag: gru_step, ...; vbl(shape) -> (V, B, L); slot(B, L) -> the key of the step's buffers;
    args / model / batch: the file's builders; reference(shape, p, seed, step, ...) / mults(shape, p, seed, step) /
    train_step(params, st, host batch, mult): the adapter to the numpy reference; the rest as _DEFAULTS explains."""
    missing, unknown = [k for k in _NEEDED if k not in kw], [k for k in kw if k not in _NEEDED and k not in _DEFAULTS]
    assert not missing and not unknown, (missing, unknown)
    return types.SimpleNamespace(tag=kw["stem"].replace("_", " ") + " step", **{**_DEFAULTS, **kw})


def _cached(key, make):
    if key not in _once:
        _once[key] = make()
    return _once[key]


def batch(D, shape):
    return _cached((D.stem, "batch", shape), lambda: D.batch(shape))


def reference(D, shape, p, seed, step, *more):
    """The file's reference at the model's initial weights, under the masks of (seed, step): computed once."""
    return _cached((D.stem, "reference", shape, p, seed, step) + more, lambda: D.reference(shape, p, seed, step, *more))


def host(D, shape):
    return tuple(np.asarray(a) for a in batch(D, shape))


def cuda(D, shape):
    import torch
    return D.call(tuple(torch.as_tensor(a).cuda() for a in batch(D, shape)))


def model_class(D):
    import bsarec_amd
    return getattr(bsarec_amd, D.name + "Model")


def pairwise_batch(V, L, B, U=None):
    """Padding zeros in front, and (beyond 10 rows) the collisions of the item-table gradient: an answer and a negative equal to a
    looked-up id, a row whose answer is its negative, a negative equal to another row's answer.  With ``U``: users drawn last."""
    import torch
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(1, V, (B, L), generator=g)
    ids[:5, :max(1, min(7, L - 1))] = 0
    pos = torch.randint(1, V, (B,), generator=g)
    neg = torch.randint(1, V, (B,), generator=g)
    users = None if U is None else torch.randint(0, U, (B,), generator=g)
    if B > 10:
        pos[6], neg[7] = ids[6, -1], ids[7, -1]
        neg[8] = pos[8]
        neg[9] = pos[10]
    return (ids, pos, neg) if U is None else (ids, users, pos, neg)


def block_batch(ragged_ids, V, L, B, seed):
    """Left-padded ids with a full row, a row of padding alone and a row whose first item is at L - 1; answers of which some are
    looked-up ids (of their own row and of another), so that the lookup and the head's answer term meet on a row of dE.  The
    asserts are conditions on the inputs (the seeds were chosen on the CPU so that they hold)."""
    rng = np.random.default_rng(seed)
    first = list(rng.integers(0, L, B))
    first[0], first[1], first[2] = 0, L, L - 1
    ids = ragged_ids(rng, B, L, first, V)
    ans = rng.integers(1, V, B)
    ans[0], ans[3] = ids[0, -1], ids[2, -1]
    assert ids[0].all() and not ids[1].any() and ids[2, -1] != 0 and not ids[2, :-1].any()
    assert len(np.intersect1d(np.unique(ids), np.unique(ans))) >= 2
    return ids, ans


def params64(m):
    return {k: v.detach().cpu().numpy().astype(np.float64) for k, v in m.state_dict().items()}


def first_call(D, shape, p):
    """-> (model, (args, kwargs), loss, grads, reference) of the first train = True call of a fresh model."""
    m = D.model(shape, p)
    a, kw = cuda(D, shape)
    loss, grads = m.loss_and_grads(*a, train=True, **kw)
    st = m.step_state.cpu().tolist()
    assert st[0] == D.seed and st[1] == 1 and st[2] == 0      # the step counter advanced once, Adam's t did not
    return m, (a, kw), loss, grads, reference(D, shape, p, st[0], st[1])      # the seed and counter READ BACK from the device


def check_loss_and_grads(D, shape, p, loss, grads, rloss, rgrads, both, zero_banks=False, line=None):
    """The loss, every gradient tensor and the item rows ``both`` (looked up AND in some row's head) against the reference.
    ``zero_banks``: a tensor whose reference is all zero must be exactly zero, and has no error.  -> the item-table gradient."""
    e_loss = abs(loss.item() - rloss) / abs(rloss)
    errs = {}
    for k, g in grads.items():
        if zero_banks and not rgrads[k].any():
            assert not g.any().item(), k                      # a bank none of whose cells passes: exactly zero
            continue
        errs[k] = rel_l2(g.cpu().numpy(), rgrads[k])
    g = grads["item_embeddings.weight"].cpu().numpy()
    e_both = rel_l2(g[both], rgrads["item_embeddings.weight"][both])
    print(f"{D.tag} shape {shape} p={p}: loss {loss.item():.7f} rel {e_loss:.2e} rows(lookup+head) {e_both:.2e} " +
          (line(errs) if line else " ".join(f"{k} {v:.2e}" for k, v in errs.items())))
    assert e_loss <= D.loss_gate
    for k, v in errs.items():
        assert v <= D.grad_gate, (k, v)
    assert e_both <= D.grad_gate
    return g


def second_call_tail(D, m, shape, p, call, loss, grads, again=None):
    """After the first call: the same call again (``again``: other keyword arguments that mean the same call), train = False,
    the p = 0 model, and the model's own eval path."""
    import torch
    a, kw = call
    # the same call again: the next masks at p > 0, the same bits at p = 0
    loss2, grads2 = m.loss_and_grads(*a, train=True, **(kw if again is None else again))
    assert m.step_state[1].item() == 2 and m.step_state[2].item() == 0
    same = all(torch.equal(grads[k], grads2[k]) for k in grads) and torch.equal(loss, loss2)
    assert same == (p == 0.0)
    # train = 0 draws nothing and touches no counter: the bits of the p = 0 model, whatever p
    loss0, grads0 = m.loss_and_grads(*a, **D.eval_kw, **kw)
    assert m.step_state[1].item() == 2
    if p > 0.0:
        lossz, gradsz = D.model(shape, 0.0).loss_and_grads(*a, train=True, **kw)
        assert torch.equal(loss0, lossz)
        for k in grads0:
            assert torch.equal(grads0[k], gradsz[k]), k
    if D.eval_loss is not True:
        return
    # ... and the loss of the model's own eval path, which evaluation ranks with
    m.eval()
    with torch.no_grad():
        want = m.calculate_loss(*a, **kw).item()
    e_eval = abs(loss0.item() - want) / abs(want)
    print(f"{D.tag} shape {shape} p={p}: loss(train=False) {loss0.item():.7f} calculate_loss(eval) {want:.7f} rel {e_eval:.2e}")
    assert e_eval <= D.loss_gate


def a_row_whose_answer_is_its_negative_adds_exactly_nothing(D):
    """Row 8 of the pairwise batch has answers == neg_answers: diff = 0 exactly, and its two head rows cancel in the fixed-point
    sum.  An id that ONLY that head touches stays exactly zero."""
    import torch
    V, B, L = D.vbl(1)
    m = D.model(1)
    ids, pos, neg = (t.clone() for t in batch(D, 1))
    lone = int(np.setdiff1d(np.arange(1, V), torch.cat([ids.reshape(-1), pos, neg]).numpy())[0])
    pos[8] = neg[8] = lone
    _, grads = m.loss_and_grads(ids.cuda(), pos.cuda(), neg.cuda(), train=False)
    assert not grads["item_embeddings.weight"][lone].any().item()


def three_adam_steps(D, p, wd):
    """Three train_steps on shape 1 beside three steps of the reference: the state, every parameter within the gradient gate,
    and that the parameters moved.  -> the model, for the file's own assertions on its flat arrays."""
    import torch
    from oracle import bsarec_oracle as O
    m = D.model(1, p, weight_decay=wd, **{D.flag + "_graph": False})
    before = {k: v.detach().clone() for k, v in m.state_dict().items()}
    params = params64(m)
    hb = host(D, 1)
    a, kw = cuda(D, 1)
    st = O.AdamState(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=wd)
    losses = []
    for step in range(1, 4):
        mult = D.mults(1, p, D.seed, step)
        if D.before_step is not None:
            D.before_step(params, hb, mult, (p, wd, step))
        losses.append(m.train_step(*a, **kw).item())
        rl = D.train_step(params, st, hb, mult)
        print(f"{D.adam_tag} p={p} wd={wd} step {step}: loss {losses[-1]:.7f} reference {rl:.7f}")
    assert np.isfinite(losses).all()
    state = m.step_state.cpu().tolist()
    assert state[0] == D.seed and state[1] == 3 and state[2] == 3          # the counter and ONE t for every array
    worst = (0.0, None)
    for k, q in m.named_parameters():
        e = rel_l2(q.detach().cpu().numpy(), params[k])
        worst = max(worst, (e, k))
        if D.moved is None:
            print(f"{D.adam_tag} x3 p={p} wd={wd} {k}: {e:.2e}")
        assert e <= D.grad_gate, (k, e)
        if D.moved is None:
            assert not torch.equal(q.detach(), before[k]), k                              # it moved
    if D.moved is not None:
        print(f"{D.adam_tag} x3 p={p} wd={wd}: worst parameter {worst[0]:.2e} ({worst[1]})")
    for k in D.moved or ():
        assert not torch.equal(m.state_dict()[k], before[k]), k                           # it moved
    return m


def three_steps(D, m, poison=False, calls=None):
    """Three train_steps on the batch of shape 1 (``calls``: the (args, kwargs) of each step) -> (losses, parameters after)."""
    import torch
    V, B, L = D.vbl(1)
    key = D.slot(B, L)
    calls = [cuda(D, 1)] * 3 if calls is None else calls
    losses = []
    for a, kw in calls:
        if poison:                                            # NaN in every float, all ones in every accumulator and window
            m._slot(m._step_buffers(), *(key if isinstance(key, tuple) else (key,)))["ws"].fill_(0xFF)
        losses.append(m.train_step(*a, **kw).clone())
    return torch.stack(losses), {k: v.detach().clone() for k, v in m.state_dict().items()}


def _eager(D):
    return D.model(1, 0.5, **{D.flag + "_graph": False})


def determinism_with_a_poisoned_workspace(D):
    import torch
    la, pa = three_steps(D, _eager(D))
    lb, pb = three_steps(D, _eager(D), poison=True)
    assert torch.isfinite(la).all() and torch.equal(la, lb)
    for k in pa:
        assert torch.equal(pa[k], pb[k]), k


def graph_replay_is_the_next_step(D, calls=None):
    """Three steps replayed from the model's graph against three eager ones, bit for bit.  -> (losses, parameters) of the replay."""
    import torch
    V, B, L = D.vbl(1)
    mg = D.model(1, 0.5)
    lg, pg = three_steps(D, mg, calls=calls)
    le, pe = three_steps(D, _eager(D), calls=calls)
    assert mg._fused["slots"][D.slot(B, L)]["graph"] is not None
    assert torch.equal(lg, le) and len(set(lg.tolist())) == 3      # three different masks, three different t
    for k in pg:
        assert torch.equal(pg[k], pe[k]), k
    assert mg.step_state.cpu().tolist()[1:3] == [3, 3]
    return lg, pg


def main_run_with_the_fused_step(D, monkeypatch):
    import torch
    from bsarec_amd import data as Dm, main as M

    def no_optimiser(*a, **kw):
        raise AssertionError(f"a torch optimiser was built for a fused {D.name}")
    monkeypatch.setattr(torch.optim, "Adam", no_optimiser)
    msgs = []

    class Grab(logging.Handler):
        def emit(self, rec):
            msgs.append(rec.msg)
    logger = logging.getLogger(D.stem + "_step_main")
    logger.setLevel(logging.INFO)
    logger.propagate = False
    logger.addHandler(Grab())
    seqs = Dm.synth_ml1m_like(seed=5, **D.main["synth"])
    args = M.parse_args(["--model_type", D.name, "--" + D.flag, "fused"] + D.main["argv"] + ["--epochs", "2", "--patience", "100"])
    scores, info, epochs, secs = M.run(args, seqs, logger)
    losses = [float(ast.literal_eval(m)["rec_loss"]) for m in msgs if isinstance(m, str) and "'rec_loss'" in m]
    print(f"{D.main['tag']}: losses {losses} scores {scores}")
    assert epochs == 2 and len(losses) == 2 and np.isfinite(losses).all()
    assert losses[1] < losses[0]
    assert len(scores) == 6 and np.isfinite(scores).all() and all(0.0 <= s <= 1.0 for s in scores)


def _refusals(D):
    """A bogus mode is refused at construction; the default mode has no train_step of its own."""
    Model = model_class(D)
    with pytest.raises(ValueError, match=D.flag):
        Model(D.args(1, **{D.flag: "bogus"}))
    default = Model(D.args(1, **{D.flag: "torch"})).cuda()
    a, kw = cuda(D, 1)
    with pytest.raises(RuntimeError, match="torch.optim.Adam"):
        default.train_step(*a, **kw)
    return Model


def _save_change_load(D, tr, model, tmp_path):
    """Checkpoint: bit for bit back into the flat arrays.  -> (path, the saved values)."""
    import torch
    path = str(tmp_path / (D.stem + "_fused.pt"))
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    tr.save(path)
    with torch.no_grad():
        for q in model.parameters():
            q.add_(1.0)
    tr.load(path)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
    return path, before


def _trains_on(tr, model, before, t):
    import torch
    tr.train(1)                                               # the step still updates the loaded arrays in place
    assert model.step_state[2].item() > t
    assert any(not torch.equal(v, before[k]) for k, v in model.state_dict().items())


def trainer_mode_switch_and_checkpoint_round_trip(D, tmp_path):
    """The pairwise models: the fused mode through the Trainer, a checkpoint, and the default mode through a torch optimiser."""
    import torch
    _refusals(D)
    _setup = importlib.import_module(D.trainer[0])._setup
    seqs, args, model, tr = _setup(["--" + D.flag, "fused"])
    assert getattr(model, D.flag) == "fused" and model.torch_optim is False
    tr.train(0)
    assert getattr(tr, "_torch_opt", None) is None
    assert model.step_state[2].item() > 0                     # Adam's t: the steps ran in the library
    path, before = _save_change_load(D, tr, model, tmp_path)
    _trains_on(tr, model, before, model.step_state[2].item())
    # the default path still trains, through a torch optimiser
    seqs, args, model, tr = _setup(["--" + D.flag, "torch"])
    assert getattr(model, D.flag) == "torch" and model.torch_optim is True
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    post = tr.train(0)
    assert np.isfinite(float(post["rec_loss"])) and getattr(tr, "_torch_opt", None) is not None
    assert not torch.equal(model.state_dict()[D.trainer[1]], before[D.trainer[1]])


def trainer_evaluation_paths_and_checkpoint_round_trip(D, tmp_path):
    """The block models: the fused mode through the Trainer, the three evaluation paths, a checkpoint into both modes."""
    import torch
    Model = _refusals(D)
    seqs, args, model, tr, test_dl = importlib.import_module(D.trainer[0])._setup(["--" + D.flag, "fused"])
    model = tr.model
    assert getattr(model, D.flag) == "fused" and model.torch_optim is False and model.own_train_step is True
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
    path, before = _save_change_load(D, tr, model, tmp_path)
    setattr(args, D.flag, "torch")
    other = Model(args).cuda()
    other.load_state_dict(torch.load(path))
    for k, v in other.state_dict().items():
        assert torch.equal(v, before[k]), k
    other.eval()
    model.eval()
    some = next(iter(test_dl))[1]
    assert torch.equal(other.last_hidden(some), model.last_hidden(some))
    _trains_on(tr, model, before, t)
