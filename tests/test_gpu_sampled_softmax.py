"""The sampled-softmax training head on the MI355X (``bsarec_config_t.train_negatives``, csrc/sampled_softmax.h):
* candidates bit-equal to the numpy restatement (tests/sampled_softmax_ref.py), fresh every step;
* loss, loss rows and dlogits against float64 on the kernel's own h_last and candidates, accidental hits included;
* every gradient against the CPU oracle with the restated head (fused and generic shapes, dropout off and on);
* eager steps == the indexed multi-step graph bit for bit, and two fresh runs are identical;
* main.run end to end, and the refusals of the C entry points."""
import argparse
import ast
import ctypes as C
import logging

import numpy as np
import pytest

import sampled_softmax_ref as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def ns(**kw):
    a = argparse.Namespace(item_size=97, hidden_size=64, max_seq_length=50, batch_size=256, hidden_dropout_prob=0.0,
                           attention_probs_dropout_prob=0.0, num_hidden_layers=2, num_attention_heads=2,
                           hidden_act="gelu", initializer_range=0.02, c=3, alpha=0.9, seed=42, lr=1e-3,
                           adam_beta1=0.9, adam_beta2=0.999, weight_decay=0.0, no_cuda=False, log_freq=1)
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


def _model(V, N, sampler="uniform", logq=True, counts=None, **kw):
    from bsarec_amd import BSARecModel
    extra = {} if logq else {"train_no_logq": True}
    m = BSARecModel(ns(item_size=V, train_negatives=N, train_sampler=sampler, **extra, **kw)).cuda()
    if sampler == "popularity" and counts is not None:
        m.set_train_popularity(counts)
    m.train()
    m.set_seed(77)
    return m


def _views(m, B, N):
    from bsarec_amd import _lib as Lb
    plan = m._plan(B)
    off = plan.lib.bsarec_buffer_offset(plan.handle, Lb.BUF_TRAIN_CAND, 0)
    cand = plan.ws[off:off + 4 * N].view(torch.int32).cpu().numpy().astype(np.int64)
    lg = plan.view(Lb.BUF_TRAIN_LOGITS, 0, (B, N + 1)).cpu().numpy()
    dl = plan.view(Lb.BUF_TRAIN_DLOGITS, 0, (B, N + 1)).cpu().numpy()
    rows = plan.view(Lb.BUF_LOSS_ROWS, 0, (B,)).cpu().numpy()
    corr = plan.view(Lb.BUF_TRAIN_CORR, 0, (N,)).cpu().numpy()
    return plan, cand, corr, lg, dl, rows


@pytest.mark.parametrize("sampler", ["uniform", "popularity"])
@pytest.mark.parametrize("V", [40, 3417, 1000003])
def test_candidates_match_the_restatement(V, sampler):
    rng = np.random.default_rng(V)
    counts = _counts(V, rng) if sampler == "popularity" else None
    cum = R.cumulative(counts) if counts is not None else None
    B, L = 4, 8
    for N in (1, 100, 8192):
        m = _model(V, N, sampler, counts=counts, hidden_size=16, max_seq_length=L, num_hidden_layers=1, num_attention_heads=1)
        ids = torch.from_numpy(_batch(V, B, L, rng)).cuda()
        ans = rng.integers(1, V, size=B).astype(np.int64)
        if cum is not None:
            ans = rng.choice(np.flatnonzero(counts), size=B).astype(np.int64)
        seen = []
        for step in (1, 2):                               # eager calculate_loss: step_begin first, so steps 1, 2
            loss = m.calculate_loss(ids, torch.from_numpy(ans).cuda(), None, None, None)
            assert np.isfinite(loss.item())
            _, cand, corr, _, _, _ = _views(m, B, N)
            want = R.draws(77, step, V, N, cum)
            np.testing.assert_array_equal(cand, want, err_msg=f"V={V} N={N} {sampler} step {step}")
            np.testing.assert_allclose(corr, R.corrections(want, N, cum).astype(np.float32), rtol=1e-6, atol=1e-6)
            if cum is not None:
                assert (counts[cand] > 0).all()
            else:
                assert ((cand >= 1) & (cand < V)).all()
            seen.append(cand)
        if N >= 100:
            assert not np.array_equal(seen[0], seen[1])


@pytest.mark.parametrize("case", ["uniform", "pop_logq", "pop_no_logq", "tiny_hits", "generic"])
def test_head_numerics_against_float64(case):
    V, N, B = 3417, 1000, 256
    kw = {}
    sampler, logq = "uniform", True
    if case.startswith("pop"):
        sampler, logq = "popularity", case == "pop_logq"
    if case == "tiny_hits":
        V, N, B = 5, 64, 32
    if case == "generic":
        kw = dict(hidden_size=48, max_seq_length=20, num_attention_heads=2)
    rng = np.random.default_rng(3)
    counts = _counts(V, rng, 0.2) if sampler == "popularity" else None
    cum = R.cumulative(counts) if counts is not None else None
    m = _model(V, N, sampler, logq, counts, **kw)
    Lq, d = m.args.max_seq_length, m.args.hidden_size
    ids = torch.from_numpy(_batch(V, B, Lq, rng)).cuda()
    ans = (rng.choice(np.flatnonzero(counts), size=B) if counts is not None else rng.integers(1, V, size=B)).astype(np.int64)
    loss = m.calculate_loss(ids, torch.from_numpy(ans).cuda(), None, None, None).item()
    plan, cand, _, lg, dl, rows = _views(m, B, N)
    from bsarec_amd import _lib as Lb
    h = plan.view(Lb.BUF_LAYER_OUT, m.args.num_hidden_layers, (B, Lq, d))[:, Lq - 1].cpu().numpy()
    E = m.item_embeddings.weight.detach().cpu().numpy()
    np.testing.assert_array_equal(cand, R.draws(77, 1, V, N, cum))
    x, lr, l64, g = R.head(h, E, ans, cand, cum, logq)
    fin = np.isfinite(x)
    assert (np.isfinite(lg) == fin).all() and (lg[~fin] == -np.inf).all()
    assert np.abs(lg[fin] - x[fin]).max() <= 1e-5 * np.abs(x[fin]).max()
    assert np.abs(rows - lr).max() <= 1e-5 * np.abs(lr).max()
    assert abs(loss - l64) <= 1e-5 * abs(l64)
    assert np.abs(dl - g).max() <= 1e-5 * np.abs(g).max()
    assert (dl[~fin] == 0).all()
    if case == "tiny_hits":
        assert (~fin).sum() > 0 and np.isfinite(loss)


def _parity_case(fused, dropout, sampler):
    from oracle import bsarec_oracle as O
    from bsarec_amd import BSARecModel
    V, N, B = 500, 128, 37
    if fused:
        cfg = O.Config(item_size=V, hidden_size=64, max_seq_length=50, num_hidden_layers=2, num_attention_heads=2, c=5, alpha=0.7,
                       hidden_dropout_prob=0.4 if dropout else 0.0, attention_probs_dropout_prob=0.3 if dropout else 0.0)
    else:
        cfg = O.Config(item_size=V, hidden_size=32, max_seq_length=20, num_hidden_layers=2, num_attention_heads=2, c=5, alpha=0.7,
                       hidden_dropout_prob=0.4 if dropout else 0.0, attention_probs_dropout_prob=0.3 if dropout else 0.0)
    params = O.init_params(cfg, seed=11)
    rng = np.random.default_rng(5)
    for k in params:
        if k.endswith(".bias"):
            params[k] = (rng.standard_normal(params[k].shape) * 0.05).astype(np.float32)
        elif "LayerNorm.weight" in k:
            params[k] = (1 + rng.standard_normal(params[k].shape) * 0.1).astype(np.float32)
    params["item_embeddings.weight"] = (rng.standard_normal(params["item_embeddings.weight"].shape) * 0.5).astype(np.float32)
    ids = _batch(V, B, cfg.max_seq_length, rng)
    counts = _counts(V, rng, 0.2) if sampler == "popularity" else None
    cum = R.cumulative(counts) if counts is not None else None
    ans = (rng.choice(np.flatnonzero(counts), size=B) if counts is not None else rng.integers(1, V, size=B)).astype(np.int64)
    a = ns(item_size=V, hidden_size=cfg.hidden_size, max_seq_length=cfg.max_seq_length, num_hidden_layers=2, num_attention_heads=2,
           c=5, alpha=0.7, hidden_dropout_prob=cfg.hidden_dropout_prob, attention_probs_dropout_prob=cfg.attention_probs_dropout_prob,
           train_negatives=N, train_sampler=sampler)
    m = BSARecModel(a)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
    m = m.cuda()
    if counts is not None:
        m.set_train_popularity(counts)
    m.train()
    m.set_seed(77)
    loss = m.calculate_loss(torch.from_numpy(ids).cuda(), torch.from_numpy(ans).cuda(), None, None, None)
    loss.backward()
    cand = R.draws(77, 1, V, N, cum)
    oloss, _, G, _ = O.loss_and_grads(params, cfg, ids, ans, O.DropoutSpec(dropout, 77, 1), head=R.oracle_head(ans, cand, cum))
    return m, loss.item(), oloss, G


@pytest.mark.parametrize("sampler", ["uniform", "popularity"])
@pytest.mark.parametrize("dropout", [False, True])
@pytest.mark.parametrize("fused", [True, False])
def test_all_gradients_match_the_oracle(fused, dropout, sampler):
    m, loss, oloss, G = _parity_case(fused, dropout, sampler)
    assert abs(loss - oloss) <= 5e-6 * abs(oloss), (loss, oloss)
    got = m.grad_views()
    assert set(got) == set(G) and len(G) == 42
    bad = {}
    for k, r in G.items():
        g = got[k].cpu().numpy()
        assert np.isfinite(g).all(), k
        if k.endswith("key.bias"):                       # true gradient is zero
            assert np.abs(g).max() <= 1e-6, k
            continue
        if rel_l2(g, r) > 2e-5:
            bad[k] = rel_l2(g, r)
    assert not bad, bad
    E_rows = np.abs(G["item_embeddings.weight"]).sum(axis=1) > 0        # rows that are no candidate and no lookup: exactly 0
    assert (got["item_embeddings.weight"].cpu().numpy()[~E_rows] == 0).all()


def _train_data(V, n, L, rng):
    inputs = _batch(V, n, L, rng)
    answers = rng.integers(1, V, size=n).astype(np.int64)
    return np.arange(n, dtype=np.int64), inputs, answers


def test_indexed_graph_steps_equal_eager_steps_bit_for_bit():
    from bsarec_amd import BSARecModel
    from bsarec_amd.data import DeviceBatches
    from bsarec_amd.trainer import Trainer
    V, B, k, L = 3000, 64, 6, 50
    rng = np.random.default_rng(9)
    u, x, a = _train_data(V, B * k, L, rng)
    args = ns(item_size=V, train_negatives=512, hidden_dropout_prob=0.3, attention_probs_dropout_prob=0.2, batch_size=B)
    torch.manual_seed(0)
    mi = BSARecModel(args)
    me = BSARecModel(args)
    me.load_state_dict(mi.state_dict())
    dl = DeviceBatches(u, x, a, B, torch.device("cuda"), shuffle=False)
    init = {kk: v.clone() for kk, v in mi.state_dict().items()}
    tr = Trainer(mi, dl, None, None, args)
    mi.set_seed(5)
    mi.train()
    mi._step_begun = True                                # eager steps use step 1, 2, ...: the indexed ones start at 1 too
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
    for (kk, p), (_, q) in zip(mi.state_dict().items(), me.state_dict().items()):
        assert torch.equal(p, q), kk
    assert not torch.equal(me.state_dict()["item_embeddings.weight"].cpu(), init["item_embeddings.weight"])


def test_two_fresh_runs_are_identical():
    from bsarec_amd import BSARecModel
    V, B, L = 20011, 128, 50
    rng = np.random.default_rng(4)
    ids = torch.from_numpy(_batch(V, B, L, rng)).cuda()
    counts = _counts(V, rng, 0.1)
    ans = torch.from_numpy(rng.choice(np.flatnonzero(counts), size=B).astype(np.int64)).cuda()   # answers the sampler can draw
    out = []
    for _ in range(2):
        torch.manual_seed(1)
        m = BSARecModel(ns(item_size=V, train_negatives=2048, train_sampler="popularity", hidden_dropout_prob=0.3)).cuda()
        m.set_train_popularity(counts)
        m.configure_adam()
        m.set_seed(21)
        m.train()
        for _ in range(4):
            m.train_step(ids, ans)
        out.append({k: v.clone() for k, v in m.state_dict().items()})
    for k in out[0]:
        assert torch.equal(out[0][k], out[1][k]), k


def _run_main(argv, epochs=3):
    from bsarec_amd import main as M
    rng = np.random.default_rng(0)
    seqs = [rng.integers(1, 400, size=int(rng.integers(5, 40))).tolist() for _ in range(200)]
    seqs[0].append(399)
    msgs = []

    class Grab(logging.Handler):
        def emit(self, rec):
            msgs.append(rec.msg)
    logger = logging.getLogger("sampled_softmax_main_" + "_".join(argv))
    logger.setLevel(logging.INFO)
    logger.propagate = False
    logger.addHandler(Grab())
    args = M.parse_args(["--epochs", str(epochs), "--batch_size", "64", "--num_attention_heads", "1", "--patience", "100"] + argv)
    scores, _, _, _ = M.run(args, seqs, logger)
    return scores, msgs


def test_main_run_trains_with_the_sampled_head():
    scores, msgs = _run_main(["--train_negatives", "128"])
    losses = [float(ast.literal_eval(m)["rec_loss"]) for m in msgs if isinstance(m, str) and "'rec_loss'" in m]
    assert len(losses) == 3 and np.isfinite(losses).all()
    assert losses[-1] < losses[0]
    assert len(scores) == 6 and np.isfinite(scores).all()
    evals = [m for m in msgs if isinstance(m, dict) and "HR@5" in m]
    assert evals and all(list(m) == ["Epoch", "HR@5", "NDCG@5", "HR@10", "NDCG@10", "HR@20", "NDCG@20"] for m in evals)


def test_main_run_without_the_flag_logs_as_before():
    scores, msgs = _run_main(["--train_negatives", "128", "--train_sampler", "popularity"], epochs=1)
    assert len(scores) == 6 and np.isfinite(scores).all()
    _, without = _run_main([], epochs=1)
    assert not any("train_negatives" in str(m) or "train_sampler" in str(m) for m in without)
    for m in without:
        if isinstance(m, str) and "'rec_loss'" in m:
            assert list(ast.literal_eval(m)) == ["epoch", "rec_loss"]
        elif isinstance(m, dict):
            assert list(m) == ["Epoch", "HR@5", "NDCG@5", "HR@10", "NDCG@10", "HR@20", "NDCG@20"]


def test_entry_points_refuse():
    from bsarec_amd import BSARecModel, _lib as Lb
    lib = Lb.load()
    V, B, L = 300, 16, 50
    rng = np.random.default_rng(2)
    ids = torch.from_numpy(_batch(V, B, L, rng)).cuda()
    ans = torch.from_numpy(rng.integers(1, V, size=B).astype(np.int64)).cuda()
    # storage = 1: no plan (the C library refuses the configuration)
    m = _model(V, 64)
    cfg = Lb.Config.from_buffer_copy(m._plan(B).cfg)
    cfg.storage = 1
    assert lib.bsarec_workspace_bytes(C.byref(cfg)) == 0
    assert lib.bsarec_config_is_fused(C.byref(cfg)) < 0
    # the bucketed dense-gradient hook and the lookup_grad buffer
    plan = m._plan(B)
    buf = torch.zeros(V * 64, device="cuda")
    assert lib.bsarec_plan_set_dense_grad_hook(plan.handle, Lb.HOOK(0), None, buf.data_ptr()) < 0
    hook = Lb.HOOK(lambda u, s: None)
    assert lib.bsarec_plan_set_dense_grad_hook(plan.handle, hook, None, None) < 0
    # backward of forward() (ext_dy)
    st = m._stream()
    assert lib.bsarec_forward(plan.handle, ids.data_ptr(), 1, st) == 0
    dy = torch.zeros(B, L, 64, device="cuda")
    assert lib.bsarec_backward_seq(plan.handle, dy.data_ptr(), st) < 0
    # popularity without a table: every loss entry point refuses before launching
    mp = _model(V, 64, "popularity")
    pp = mp._plan(B)
    assert lib.bsarec_loss(pp.handle, ans.data_ptr(), st) < 0
    mp.configure_adam()
    ad = mp._adam_struct()
    assert lib.bsarec_train_step(pp.handle, ids.data_ptr(), ans.data_ptr(), C.byref(ad), st) < 0
    assert lib.bsarec_plan_set_train_sampler(plan.handle, None) < 0          # a uniform plan has no table to take
    torch.cuda.synchronize()
    with pytest.raises(RuntimeError):
        mp.calculate_loss(ids, ans, None, None, None)
