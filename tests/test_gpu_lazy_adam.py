"""Lazy (sparse) Adam for the item table on the MI355X (``bsarec_config_t.train_lazy_adam``, csrc/lazy_adam.h):
* the first step from fresh moments equals the dense step bit for bit (eager and fused indexed steps, fused and generic
  shapes);
* several steps against the numpy restatement (tests/lazy_adam_ref.py): touched rows match, untouched rows of w, m, v and
  of the gradient arena unchanged bit for bit -- with weight decay, the popularity sampler, heavy duplicates and V = 1,000,003;
* captured indexed steps equal eager steps bit for bit; main.run end to end; the refusals of the C entry points."""
import argparse
import ast
import ctypes as C
import logging

import numpy as np
import pytest

import lazy_adam_ref as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def ns(**kw):
    a = argparse.Namespace(item_size=97, hidden_size=64, max_seq_length=50, batch_size=256, hidden_dropout_prob=0.0,
                           attention_probs_dropout_prob=0.0, num_hidden_layers=2, num_attention_heads=2,
                           hidden_act="gelu", initializer_range=0.02, c=3, alpha=0.9, seed=42, lr=LR,
                           adam_beta1=B1, adam_beta2=B2, weight_decay=0.0, no_cuda=False, log_freq=1)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _counts(V, rng, zero_frac=0.3):
    c = rng.integers(1, 50, size=V).astype(np.int64)
    c[rng.random(V) < zero_frac] = 0
    c[0] = 0
    c[1] = max(c[1], 1)
    return c


def _batch(V, B, L, rng):
    ids = rng.integers(1, V, size=(B, L)).astype(np.int64)
    ids[rng.random((B, L)) < 0.3] = 0
    return ids


def _pair(V, N, wd=0.0, sampler="uniform", counts=None, **kw):
    """A dense and a lazy model with the same weights, seed and Adam settings."""
    from bsarec_amd import BSARecModel
    torch.manual_seed(0)
    out = []
    for lazy in (False, True):
        m = BSARecModel(ns(item_size=V, train_negatives=N, train_sampler=sampler, train_lazy_adam=lazy, **kw))
        if out:
            m.load_state_dict(out[0].state_dict())
        m = m.cuda()
        if counts is not None:
            m.set_train_popularity(counts)
        m.configure_adam(lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd)
        m.set_seed(77)
        m.train()
        out.append(m)
    return out


def _cand(m, B, N):
    from bsarec_amd import _lib as Lb
    plan = m._plan(B)
    off = plan.lib.bsarec_buffer_offset(plan.handle, Lb.BUF_TRAIN_CAND, 0)
    return plan.ws[off:off + 4 * N].view(torch.int32).cpu().numpy().astype(np.int64)


def _item(m, arena):
    o, n, shp = m._slices["item_embeddings.weight"]
    return arena[o:o + n].view(shp)


def _answers(V, B, rng, counts):
    if counts is not None:
        return rng.choice(np.flatnonzero(counts), size=B).astype(np.int64)
    return rng.integers(1, V, size=B).astype(np.int64)


def _indexed(m, ids, ans):
    """One bsarec_train_step_indexed over a one-batch table (the fused reduce + Adam launch at the fused shape)."""
    B = ids.shape[0]
    table, at = torch.from_numpy(ids).cuda(), torch.from_numpy(ans).cuda()
    perm = torch.arange(B, dtype=torch.int64, device="cuda")
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    m._step_begun = True
    return m.train_step_indexed(table, at, perm, cursor, B)


@pytest.mark.parametrize("path", ["eager", "indexed"])
@pytest.mark.parametrize("shape", ["fused", "generic_d128", "no_fused"])
def test_first_step_equals_dense_bit_for_bit(shape, path):
    kw = {}
    if shape == "generic_d128":
        kw = dict(hidden_size=128, max_seq_length=20)
    if shape == "no_fused":
        kw = dict(plan_options={"no_fused": 1})
    V, N, B = 3001, 256, 128
    dense, lazy = _pair(V, N, batch_size=B, **kw)
    L = dense.args.max_seq_length
    rng = np.random.default_rng(1)
    ids, ans = _batch(V, B, L, rng), rng.integers(1, V, size=B).astype(np.int64)
    for m in (dense, lazy):
        if path == "eager":
            m.train_step(torch.from_numpy(ids).cuda(), torch.from_numpy(ans).cuda())
        else:
            _indexed(m, ids, ans)
    torch.cuda.synchronize()
    cand = _cand(lazy, B, N)
    assert np.array_equal(cand, _cand(dense, B, N))
    T = torch.from_numpy(R.touched(ids, ans, cand, V)).cuda()
    for (k, p), (_, q) in zip(dense.state_dict().items(), lazy.state_dict().items()):
        assert torch.equal(p, q), k
    for key in ("m", "v"):
        assert torch.equal(dense._adam[key], lazy._adam[key]), key
    gd, gl = dense.grad_views(), lazy.grad_views()
    for k in gd:
        if k == "item_embeddings.weight":
            assert torch.equal(gd[k][T], gl[k][T])
        else:
            assert torch.equal(gd[k], gl[k]), k
    assert (gl["item_embeddings.weight"][T].abs().sum(1) > 0).any()


def _steps_against_restatement(V, N, B, steps, wd=0.0, sampler="uniform", path="eager", seed=3):
    from bsarec_amd import BSARecModel
    rng = np.random.default_rng(seed)
    counts = _counts(V, rng, 0.2) if sampler == "popularity" else None
    torch.manual_seed(0)
    m = BSARecModel(ns(item_size=V, train_negatives=N, train_sampler=sampler, train_lazy_adam=True, batch_size=B)).cuda()
    if counts is not None:
        m.set_train_popularity(counts)
    m.configure_adam(lr=LR, betas=(B1, B2), eps=EPS, weight_decay=wd)
    m.set_seed(77)
    m.train()
    L = m.args.max_seq_length
    W, M_, V_, G = _item(m, m._arena), _item(m, m._adam["m"]), _item(m, m._adam["v"]), _item(m, m._garena)
    for t in range(1, steps + 1):
        w0, m0, v0, g0 = W.clone(), M_.clone(), V_.clone(), G.clone()
        ids, ans = _batch(V, B, L, rng), _answers(V, B, rng, counts)
        if path == "eager":
            m.train_step(torch.from_numpy(ids).cuda(), torch.from_numpy(ans).cuda())
        else:
            _indexed(m, ids, ans)
        torch.cuda.synchronize()
        cand = _cand(m, B, N)
        T = R.touched(ids, ans, cand, V)
        Tt = torch.from_numpy(T).cuda()
        out = torch.ones(V, dtype=torch.bool, device="cuda")
        out[Tt] = False
        for name, now, before in (("w", W, w0), ("m", M_, m0), ("v", V_, v0), ("grad", G, g0)):
            assert torch.equal(now[out], before[out]), f"step {t}: untouched rows of {name} changed"
        g = G[Tt].cpu().numpy()
        w_, m_, v_ = (x[Tt].cpu().numpy() for x in (w0, m0, v0))
        rows = np.arange(len(T))
        ew, em, ev = R.lazy_step(w_, m_, v_, g, rows, t, LR, B1, B2, EPS, wd)
        for name, now, want in (("w", W, ew), ("m", M_, em), ("v", V_, ev)):
            got = now[Tt].cpu().numpy()
            assert rel_l2(got, want) <= 1e-6, (t, name, rel_l2(got, want))
        assert not np.array_equal(W[Tt].cpu().numpy(), w_), f"step {t}: no touched row moved"
    return m


@pytest.mark.parametrize("case", [
    dict(V=301, N=128, B=64, wd=0.01),
    dict(V=301, N=128, B=64, sampler="popularity"),
    dict(V=301, N=128, B=64, wd=0.01, path="indexed"),
    dict(V=100003, N=1024, B=256),
    dict(V=100003, N=1024, B=256, wd=0.01, sampler="popularity", path="indexed"),
])
def test_several_steps_against_the_restatement(case):
    _steps_against_restatement(steps=5, **case)


@pytest.mark.parametrize("path", ["eager", "indexed"])
def test_duplicates_update_each_row_once(path):
    # V = 41 with 64 x 50 ids, 64 answers and 512 candidates: every item occurs many times in T's sources
    _steps_against_restatement(41, 512, 64, 4, wd=0.01, path=path, seed=8)


def test_large_catalogue():
    _steps_against_restatement(1000003, 1024, 256, 3, path="indexed", seed=5)


def _train_data(V, n, L, rng):
    inputs = _batch(V, n, L, rng)
    answers = rng.integers(1, V, size=n).astype(np.int64)
    return np.arange(n, dtype=np.int64), inputs, answers


def test_graph_replay_equals_eager_bit_for_bit():
    from bsarec_amd import BSARecModel
    from bsarec_amd.data import DeviceBatches
    from bsarec_amd.trainer import Trainer
    V, B, k, L = 3000, 64, 8, 50
    rng = np.random.default_rng(9)
    u, x, a = _train_data(V, B * k, L, rng)
    args = ns(item_size=V, train_negatives=512, train_lazy_adam=True, hidden_dropout_prob=0.3,
              attention_probs_dropout_prob=0.2, batch_size=B, weight_decay=0.01)
    torch.manual_seed(0)
    mi = BSARecModel(args)
    me = BSARecModel(args)
    me.load_state_dict(mi.state_dict())
    dl = DeviceBatches(u, x, a, B, torch.device("cuda"), shuffle=False)
    tr = Trainer(mi, dl, None, None, args)
    mi.set_seed(5)
    mi.train()
    mi._step_begun = True
    perm = torch.arange(B * k, dtype=torch.int64, device="cuda")
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    tr.indexed_steps(dl, perm, cursor, None, k)
    me = me.cuda()
    me.configure_adam(lr=args.lr, betas=(args.adam_beta1, args.adam_beta2), weight_decay=args.weight_decay)
    me.set_seed(5)
    me.train()
    for s in range(k):
        me.train_step(dl.inputs[s * B:(s + 1) * B], dl.answers[s * B:(s + 1) * B])
    torch.cuda.synchronize()
    assert tr.graphs_built() > 0
    for (kk, p), (_, q) in zip(mi.state_dict().items(), me.state_dict().items()):
        assert torch.equal(p, q), kk
    for key in ("m", "v"):
        assert torch.equal(mi._adam[key], me._adam[key]), key


def test_entry_points_refuse():
    from bsarec_amd import BSARecModel, _lib as Lb
    lib = Lb.load()
    V, B, L, N = 300, 16, 50, 64
    rng = np.random.default_rng(2)
    m = BSARecModel(ns(item_size=V, train_negatives=N, train_lazy_adam=True, batch_size=B)).cuda()
    m.configure_adam()
    m.set_seed(3)
    m.train()
    plan = m._plan(B)
    st = m._stream()
    table = torch.from_numpy(_batch(V, B, L, rng)).cuda()
    at = torch.from_numpy(rng.integers(1, V, size=B).astype(np.int64)).cuda()
    perm = torch.arange(B, dtype=torch.int64, device="cuda")
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    ids_buf = torch.zeros((B, L), dtype=torch.int64, device="cuda")
    ans_buf = torch.zeros(B, dtype=torch.int64, device="cuda")
    m._garena.fill_(0.5)
    before = (m._arena.clone(), m._garena.clone(), m._state.clone())
    torch.cuda.synchronize()
    assert lib.bsarec_grad_step_indexed(plan.handle, table.data_ptr(), at.data_ptr(), perm.data_ptr(), B, cursor.data_ptr(),
                                        ids_buf.data_ptr(), ans_buf.data_ptr(), 1e-3, 0.9, 0.999, st) < 0
    # an Adam struct whose flat arena does not hold the item table
    ad = m._adam_struct()
    o = m._slices["item_embeddings.weight"][0]
    ad.n = o if o > 0 else 4
    assert lib.bsarec_train_step(plan.handle, table.data_ptr(), at.data_ptr(), C.byref(ad), st) < 0
    ad = m._adam_struct()
    ad.grads2, ad.grads2_n = m._garena.data_ptr(), 4
    assert lib.bsarec_train_step_indexed(plan.handle, table.data_ptr(), at.data_ptr(), perm.data_ptr(), B, cursor.data_ptr(),
                                         ids_buf.data_ptr(), ans_buf.data_ptr(), C.byref(ad), st) < 0
    torch.cuda.synchronize()
    for x, y in zip(before, (m._arena, m._garena, m._state)):
        assert torch.equal(x, y)
    assert cursor.item() == 0
    # the plan refuses a lazy configuration without a sampled head
    cfg = Lb.Config.from_buffer_copy(plan.cfg)
    assert cfg.train_lazy_adam == 1
    cfg.train_negatives = 0
    assert lib.bsarec_workspace_bytes(C.byref(cfg)) == 0
    with pytest.raises(ValueError):
        m.adam_step()


def test_loss_and_backward_on_a_lazy_plan_equal_the_plain_plan():
    """The autograd path (bsarec_loss + bsarec_backward) of a lazy plan computes and stores what a plan without the flag does."""
    V, N, B = 2003, 256, 64
    dense, lazy = _pair(V, N, batch_size=B)
    rng = np.random.default_rng(4)
    ids = torch.from_numpy(_batch(V, B, 50, rng)).cuda()
    ans = torch.from_numpy(rng.integers(1, V, size=B).astype(np.int64)).cuda()
    for m in (dense, lazy):
        m.calculate_loss(ids, ans, None, None, None).backward()
    torch.cuda.synchronize()
    for k, g in dense.grad_views().items():
        assert torch.equal(g, lazy.grad_views()[k]), k
    # and a lazy step after it still updates exactly its own touched rows
    lazy.train_step(ids, ans)
    dense.train_step(ids, ans)
    torch.cuda.synchronize()
    assert torch.isfinite(lazy._arena).all()


def test_main_run_end_to_end():
    from bsarec_amd import main as M
    rng = np.random.default_rng(0)
    seqs = [rng.integers(1, 400, size=int(rng.integers(5, 40))).tolist() for _ in range(200)]
    seqs[0].append(399)
    msgs = []

    class Grab(logging.Handler):
        def emit(self, rec):
            msgs.append(rec.msg)
    logger = logging.getLogger("lazy_adam_main")
    logger.setLevel(logging.INFO)
    logger.propagate = False
    logger.addHandler(Grab())
    args = M.parse_args(["--epochs", "2", "--batch_size", "64", "--num_attention_heads", "1", "--patience", "100",
                         "--train_negatives", "64", "--train_lazy_adam"])
    assert args.train_lazy_adam is True
    scores, _, _, _ = M.run(args, seqs, logger)
    losses = [float(ast.literal_eval(m)["rec_loss"]) for m in msgs if isinstance(m, str) and "'rec_loss'" in m]
    assert len(losses) == 2 and np.isfinite(losses).all()
    assert len(scores) == 6 and np.isfinite(scores).all()
