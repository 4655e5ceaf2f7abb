"""Sampled-candidate evaluation on the MI355X (``bsarec_sampled_rank`` and its path up to main.run).

* candidates bit-equal to the numpy restatement (tests/sampled_eval_ref.py), uniform and popularity, V in {40, 3417,
  1000003}, N in {1, 100, 1024} where the pool allows it, seen rows empty / holding the answer / long (global-memory
  search) / leaving exactly N eligible items; every candidate list obeys the acceptance rule;
* candidates independent of the batch: B = 1, 7, 256 and a shuffled order;
* scores against float64 dot products, ranks against the protocol's rule on the kernel's own scores and against float64
  ranks away from near ties, with +-inf and NaN in h;
* a row with too few eligible items: ValueError from the Trainer, rank -1 from the raw entry point;
* N = V - 2 without a seen set equals the full sort (full_logits + bsarec_topk_seen);
* Trainer.valid / test and main.run end to end, and the default run's log keys unchanged.
"""
import argparse
import logging

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import sampled_eval_ref as R

NEG_SEEN_LDS = 2048          # seen rows up to this length are staged in LDS by the kernel (csrc/sampled_rank.h)


def _ptr(t):
    return None if t is None else t.data_ptr()


def run_kernel(h, E, users, answers, seen=None, cum=None, n=100, seed=1234, tag=1):
    """bsarec_sampled_rank on numpy inputs.  seen: list of sorted item arrays, one CSR row per user id (users index it), or
    None (indptr = NULL).  Returns (rank, cand, score) as numpy."""
    from bsarec_amd import _lib as Lb
    lib = Lb.load()
    B, d = h.shape
    V = E.shape[0]
    ht = torch.as_tensor(np.ascontiguousarray(h, dtype=np.float32)).cuda()
    Et = E if torch.is_tensor(E) else torch.as_tensor(np.ascontiguousarray(E, dtype=np.float32)).cuda()
    ut = torch.as_tensor(np.asarray(users, dtype=np.int64)).cuda()
    at = torch.as_tensor(np.asarray(answers, dtype=np.int64)).cuda()
    indptr = indices = None
    if seen is not None:
        ip = np.concatenate([[0], np.cumsum([len(r) for r in seen])]).astype(np.int64)
        indptr = torch.as_tensor(ip).cuda()
        indices = torch.as_tensor(np.concatenate([np.asarray(r, np.int64) for r in seen] + [np.zeros(1, np.int64)])).cuda()
    ct = None if cum is None else torch.as_tensor(np.asarray(cum, dtype=np.int64)).cuda()
    rank = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    cand = torch.full((B, n + 1), -7, dtype=torch.int64, device="cuda")
    score = torch.empty(B, n + 1, dtype=torch.float32, device="cuda")
    Lb.check(lib.bsarec_sampled_rank(ht.data_ptr(), d, Et.data_ptr(), B, V, d, ut.data_ptr(), at.data_ptr(), _ptr(indptr),
                                     _ptr(indices), _ptr(ct), n, seed, tag, rank.data_ptr(), cand.data_ptr(), score.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream), "bsarec_sampled_rank")
    torch.cuda.synchronize()
    return rank.cpu().numpy(), cand.cpu().numpy(), score.cpu().numpy()


def _pop(V, rng):
    """Zipf-like training counts with ~20 % zeros; item 0 has none."""
    p = rng.zipf(1.6, size=V).astype(np.int64)
    p[rng.random(V) < 0.2] = 0
    p[0] = 0
    return p


def _rows(V, n, pop, rng):
    """(user row, answer, sorted seen items) of the seen-set shapes this case allows."""
    drawable = np.arange(1, V) if pop is None else np.nonzero(pop > 0)[0]
    rows = []
    a = int(rng.choice(drawable))
    rows.append((a, np.zeros(0, np.int64)))                                         # nothing seen
    short = rng.choice(np.arange(1, V), size=min(V // 4, 300), replace=False)
    rows.append((int(short[0]), np.unique(short)))                                  # holds the answer
    if V > 20000:
        rows.append((a, np.unique(rng.choice(np.arange(1, V), size=6000, replace=False))))   # long: searched in global memory
    if V >= 3417:
        for m in (NEG_SEEN_LDS, NEG_SEEN_LDS + 1):                              # last staged length, first searched one
            rows.append((a, np.unique(rng.choice(np.setdiff1d(np.arange(1, V), [a]), size=m, replace=False))))
    w = np.ones(V) if pop is None else pop.astype(np.float64)
    w[0] = 0.0
    pool = drawable[drawable != a]
    if len(pool) >= n:
        # exactly n eligible: the n heaviest items stay (uniform: any n), when the stream can collect the lightest of them
        keep = rng.choice(pool, size=n, replace=False) if pop is None else pool[np.argsort(-w[pool], kind="stable")[:n]]
        if w.sum() / w[keep].min() * (np.log(n) + 1) < R.NEG_MAX_DRAWS / 4:
            rows.append((a, np.setdiff1d(np.arange(1, V), np.concatenate([keep, [a]]))))
    out = []
    for a, s in rows:
        if R.eligible_count(a, s, V, pop) >= n:
            out.append((a, s))
    return out


CASES = [(V, n, smp) for V in (40, 3417, 1000003) for n in (1, 100, 1024) for smp in ("uniform", "popularity")
         if n <= V - 40 or n == 1]
CASES += [(40, 38, "uniform"), (40, 20, "popularity")]                            # the whole pool of a tiny catalogue


@pytest.mark.parametrize("V,n,sampler", CASES)
def test_candidates_equal_the_restatement(V, n, sampler):
    rng = np.random.default_rng(V * 7 + n)
    pop = _pop(V, rng) if sampler == "popularity" else None
    cum = None if pop is None else np.cumsum(pop)
    rows = _rows(V, n, pop, rng)
    assert rows
    d = 64
    E = torch.randn(V, d, device="cuda", generator=torch.Generator("cuda").manual_seed(V))
    users = np.arange(len(rows), dtype=np.int64)
    answers = np.array([a for a, _ in rows])
    seen = [s for _, s in rows]
    h = rng.standard_normal((len(rows), d)).astype(np.float32)
    seed, tag = 0x0123456789ABCDEF, 2
    rank, cand, score = run_kernel(h, E, users, answers, seen, cum, n, seed, tag)
    done = 0
    for b, (a, s) in enumerate(rows):
        want = R.candidates(int(users[b]), a, s, seed, tag, V, n, cum)
        if want is None:                                  # (a popularity-weighted pool the stream cannot exhaust in time)
            assert rank[b] == -1 and cand[b, 0] == a and np.isnan(score[b]).all()
            continue
        done += 1
        np.testing.assert_array_equal(cand[b], want, err_msg=f"row {b}")
        neg = cand[b, 1:]
        assert cand[b, 0] == a and neg.min() >= 1 and neg.max() < V and a not in neg
        assert not np.isin(neg, s).any() and len(np.unique(neg)) == n
        if pop is not None:
            assert (pop[neg] > 0).all()
        assert rank[b] == R.rank_of(score[b])
    assert done >= max(1, len(rows) - 2)


def test_candidates_with_64_bit_users_and_no_seen_set():
    V, n = 3417, 100
    rng = np.random.default_rng(3)
    users = np.array([0, 1, 2**32, 2**32 + 1, (2**40) + 12345, 2**63 - 1], dtype=np.int64)
    answers = rng.integers(1, V, size=len(users))
    E = rng.standard_normal((V, 64)).astype(np.float32)
    h = rng.standard_normal((len(users), 64)).astype(np.float32)
    for tag in (1, 2):
        _, cand, _ = run_kernel(h, E, users, answers, None, None, n, 99, tag)
        for b in range(len(users)):
            np.testing.assert_array_equal(cand[b], R.candidates(int(users[b]), int(answers[b]), [], 99, tag, V, n))
    assert len({tuple(c) for c in cand[:, 1:]}) == len(users)         # hi32(u) reaches the stream


@pytest.mark.parametrize("sampler", ["uniform", "popularity"])
def test_candidates_do_not_depend_on_the_batch(sampler):
    V, n, B = 3417, 100, 256
    rng = np.random.default_rng(5)
    pop = _pop(V, rng) if sampler == "popularity" else None
    cum = None if pop is None else np.cumsum(pop)
    seen = [np.unique(rng.integers(1, V, size=int(rng.integers(0, 400)))) for _ in range(B)]
    answers = rng.integers(1, V, size=B)
    if pop is not None:
        answers = rng.choice(np.nonzero(pop > 0)[0], size=B)
    E = rng.standard_normal((V, 64)).astype(np.float32)
    h = rng.standard_normal((B, 64)).astype(np.float32)
    users = np.arange(B)
    _, full, sfull = run_kernel(h, E, users, answers, seen, cum, n)
    for b in (0, 17, 255):
        _, one, s1 = run_kernel(h[b:b + 1], E, users[b:b + 1], answers[b:b + 1], seen, cum, n)
        np.testing.assert_array_equal(one[0], full[b])
        np.testing.assert_array_equal(s1[0], sfull[b])
    for s in range(0, B, 7):
        _, part, _ = run_kernel(h[s:s + 7], E, users[s:s + 7], answers[s:s + 7], seen, cum, n)
        np.testing.assert_array_equal(part, full[s:s + 7])
    perm = rng.permutation(B)
    _, shuf, _ = run_kernel(h[perm], E, users[perm], answers[perm], seen, cum, n)
    np.testing.assert_array_equal(shuf, full[perm])
    for b in (3, 100):
        np.testing.assert_array_equal(full[b], R.candidates(b, int(answers[b]), seen[b], 1234, 1, V, n, cum))


@pytest.mark.parametrize("d", [4, 64, 100, 256])
def test_scores_and_ranks(d):
    V, n, B = 3417, 1024, 64
    rng = np.random.default_rng(d)
    E = (rng.standard_normal((V, d)) * 0.5).astype(np.float32)
    h = rng.standard_normal((B, d)).astype(np.float32)
    h[1, 0] = np.inf
    h[2, 3 % d] = -np.inf
    h[3, 1] = np.nan
    h[4, 0], h[4, 1] = np.inf, -np.inf
    # rows whose answer ties with negatives: duplicate item rows
    E[100:110] = E[99]
    answers = rng.integers(1, V, size=B)
    answers[5] = 99
    rank, cand, score = run_kernel(h, E, np.arange(B), answers, None, None, n)
    E64 = E.astype(np.float64)
    for b in range(B):
        s64 = E64[cand[b]] @ h[b].astype(np.float64)
        assert rank[b] == R.rank_of(score[b]), b
        fin = np.isfinite(s64)
        np.testing.assert_array_equal(np.isnan(score[b]), np.isnan(s64))
        np.testing.assert_array_equal(score[b][np.isinf(s64)], s64[np.isinf(s64)])
        bound = np.abs(E64[cand[b]]) @ np.abs(h[b].astype(np.float64))
        assert np.all(np.abs(score[b][fin] - s64[fin]) <= 1e-5 * bound[fin] + 1e-30), b
        if fin.all() and np.min(np.abs(s64[1:] - s64[0])) > 1e-4:
            assert rank[b] == R.rank_of(s64), b
    assert rank[3] == n                                   # NaN answer score
    if np.isin(np.arange(100, 110), cand[5]).any():     # ties count against the model (E[100..109] == E[99])
        assert rank[5] >= np.isin(np.arange(100, 110), cand[5]).sum()


def _ns(**kw):
    a = argparse.Namespace(item_size=301, hidden_size=64, max_seq_length=50, batch_size=128, hidden_dropout_prob=0.0,
                           attention_probs_dropout_prob=0.0, num_hidden_layers=2, num_attention_heads=2,
                           hidden_act="gelu", initializer_range=0.02, c=3, alpha=0.9, seed=42, lr=1e-3,
                           adam_beta1=0.9, adam_beta2=0.999, weight_decay=0.0, no_cuda=False, log_freq=1)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _eval_setup(model_cls, V=301, n_users=300, **kw):
    import scipy.sparse as sp
    from bsarec_amd import data as D
    from bsarec_amd.trainer import Trainer
    rng = np.random.default_rng(7)
    L = 50
    seqs = [rng.integers(1, V, size=int(rng.integers(4, 60))).tolist() for _ in range(n_users)]
    a = _ns(item_size=V, **kw)
    dls = {}
    for split in ("valid", "test"):
        indptr, cols = D.seen_csr(seqs, split)
        setattr(a, f"{split}_rating_matrix", sp.csr_matrix((np.ones(len(cols)), cols, indptr), shape=(len(seqs), V)))
        dls[split] = D.DeviceBatches(*D.eval_table(seqs, L, split), a.batch_size, torch.device("cuda", 0), shuffle=False)
    a.item_popularity = D.item_popularity(seqs, V)
    torch.manual_seed(11)
    model = model_cls(a).cuda()
    tr = Trainer(model, None, dls["valid"], dls["test"], a, None)
    return tr, model, seqs, a


def test_too_few_eligible_items():
    from bsarec_amd import BSARecModel
    tr, model, seqs, a = _eval_setup(BSARecModel, V=301, eval_negatives=100)
    a.train_matrix = a.valid_rating_matrix
    from bsarec_amd import data as D
    users, ins, ans = D.eval_table(seqs, 50, "valid")
    # user 0 sees 250 of the 300 items: 49 or 50 eligible < 100
    big = np.setdiff1d(np.arange(1, 251), [ans[0]])
    m = a.valid_rating_matrix.tolil()
    m[0, big] = 1.0
    a.train_matrix = m.tocsr()
    x = torch.as_tensor(ins[:8]).cuda()
    with pytest.raises(ValueError, match=r"users \[0\]"):
        tr.sampled_ranks(torch.as_tensor(users[:8]).cuda(), x, torch.as_tensor(ans[:8]).cuda())
    # the raw entry point: rank -1 for that row, the others ranked
    csr = a.train_matrix
    seen = [np.sort(csr.indices[csr.indptr[u]:csr.indptr[u + 1]]).astype(np.int64) for u in range(csr.shape[0])]
    E = model.item_embeddings.weight.detach().cpu().numpy()
    h = model.last_hidden(x).float().cpu().numpy()
    rank, cand, score = run_kernel(h, E, users[:8], ans[:8], seen, None, 100)
    assert rank[0] == -1 and (rank[1:] >= 0).all()
    assert cand[0, 0] == ans[0] and np.isnan(score[0]).all()
    k = int((cand[0, 1:] != 0).sum())
    assert k == R.eligible_count(int(ans[0]), seen[0], 301) and (cand[0, 1 + k:] == 0).all()


def test_all_items_as_candidates_equal_the_full_sort():
    from bsarec_amd import BSARecModel, _lib as Lb
    V = 503
    tr, model, seqs, a = _eval_setup(BSARecModel, V=V)
    with torch.no_grad():
        for p in model.parameters():
            p.normal_(0.0, 0.5, generator=torch.Generator("cuda").manual_seed(p.numel()))
    from bsarec_amd import data as D
    users, ins, ans = D.eval_table(seqs, 50, "test")
    B = 128
    x = torch.as_tensor(ins[:B]).cuda()
    h = model.last_hidden(x).float().clone()
    scores = model.full_logits(x).clone()
    scores[:, 0] = -np.inf
    k = 100
    idx = torch.empty(B, k, dtype=torch.int64, device="cuda")
    Lb.check(Lb.load().bsarec_topk_seen(scores.data_ptr(), scores.stride(0), B, V, None, None, None, k, idx.data_ptr(), None,
                                        torch.cuda.current_stream().cuda_stream), "bsarec_topk_seen")
    E = model.item_embeddings.weight.detach()
    rank, cand, sc = run_kernel(h.cpu().numpy(), E, users[:B], ans[:B], None, None, V - 2)
    s64 = scores.double().cpu().numpy()
    idx = idx.cpu().numpy()
    full_rank = np.array([int(np.nonzero(idx[b] == ans[b])[0][0]) if (idx[b] == ans[b]).any() else k for b in range(B)])
    # rows with a score within 1e-4 of the answer's could order differently under the two kernels' roundings
    far = np.array([np.sort(np.abs(np.delete(s64[b, 1:], ans[b] - 1) - s64[b, ans[b]]))[0] > 1e-4 for b in range(B)])
    assert far.sum() >= B - 4
    assert all(sorted(cand[b, 1:].tolist()) == sorted(set(range(1, V)) - {int(ans[b])}) for b in range(B))
    r_samp = np.minimum(rank[far], k)
    for kk in (5, 10, 20, 50, 100):
        np.testing.assert_array_equal(R.metrics(r_samp, (kk,)), R.metrics(full_rank[far], (kk,)))


@pytest.mark.parametrize("model_name", ["BSARec", "SASRec"])
def test_trainer_valid_and_test_equal_the_restatement(model_name):
    from bsarec_amd.model import MODEL_DICT
    from bsarec_amd import data as D
    for sampler in ("uniform", "popularity"):
        tr, model, seqs, a = _eval_setup(MODEL_DICT[model_name.lower()], eval_negatives=100, eval_sampler=sampler,
                                         eval_seed=2024)
        cum = np.cumsum(a.item_popularity) if sampler == "popularity" else None
        for split, fn, tag in (("valid", tr.valid, 1), ("test", tr.test, 2)):
            got, txt = fn(0)
            assert f"'Protocol': '{sampler}-100'" in txt and len(got) == 6
            users, ins, ans = D.eval_table(seqs, 50, split)
            mat = getattr(a, f"{split}_rating_matrix")
            E = model.item_embeddings.weight.detach().double().cpu().numpy()
            ranks, near = [], 0
            for s in range(0, len(users), a.batch_size):
                x = torch.as_tensor(ins[s:s + a.batch_size]).cuda()
                h = model.last_hidden(x).double().cpu().numpy()
                _, cand, _ = tr.sampled_ranks(torch.as_tensor(users[s:s + a.batch_size]).cuda(), x,
                                              torch.as_tensor(ans[s:s + a.batch_size]).cuda(), return_candidates=True, tag=tag)
                cand = cand.cpu().numpy()
                for r in range(x.shape[0]):
                    u = int(users[s + r])
                    want = R.candidates(u, int(ans[s + r]), mat.indices[mat.indptr[u]:mat.indptr[u + 1]], 2024, tag, a.item_size,
                                        100, cum)
                    np.testing.assert_array_equal(cand[r], want)
                    s64 = E[want] @ h[r]
                    near += int(np.min(np.abs(s64[1:] - s64[0])) <= 1e-4)
                    ranks.append(R.rank_of(s64))
            np.testing.assert_allclose(got, R.metrics(ranks), atol=near / len(ranks) + 1e-12)


def _run_main(argv):
    from bsarec_amd import main as M
    rng = np.random.default_rng(0)
    seqs = [rng.integers(1, 400, size=int(rng.integers(5, 40))).tolist() for _ in range(200)]
    seqs[0].append(399)
    msgs = []

    class Grab(logging.Handler):
        def emit(self, rec):
            msgs.append(rec.msg)
    logger = logging.getLogger("sampled_eval_main_" + "_".join(argv))
    logger.setLevel(logging.INFO)
    logger.propagate = False
    logger.addHandler(Grab())
    args = M.parse_args(["--epochs", "1", "--batch_size", "64", "--num_attention_heads", "1"] + argv)
    scores, info, _, _ = M.run(args, seqs, logger)
    return scores, [m for m in msgs if isinstance(m, dict) and "HR@5" in m]


def test_main_run_with_sampled_evaluation():
    scores, evals = _run_main(["--eval_negatives", "100", "--eval_sampler", "popularity"])
    assert len(scores) == 6 and np.isfinite(scores).all()
    assert len(evals) == 2                               # valid epoch 0, test
    for m in evals:
        assert m["Protocol"] == "popularity-100"
        assert all(np.isfinite(float(m[k])) for k in ("HR@5", "NDCG@5", "HR@10", "NDCG@10", "HR@20", "NDCG@20"))


def test_main_run_without_the_flag_logs_todays_keys():
    scores, evals = _run_main([])
    assert len(scores) == 6 and len(evals) == 2
    for m in evals:
        assert list(m) == ["Epoch", "HR@5", "NDCG@5", "HR@10", "NDCG@10", "HR@20", "NDCG@20"]
