"""The answer-rank evaluation (bsarec_answer_rank, --eval_full_rank rank) on the host, no GPU: the numpy restatement against
the index of the answer in the full list, the additivity over contiguous ranges, the metrics from ranks against those from
the hit matrix, MRR, the flag and its refusals, and the argument checks of the three entry points (which return < 0 before
any HIP call)."""
import argparse
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import answer_rank_ref as A
import full_rank_ref as R


def _case(kind, B, V, seed):
    rng = np.random.default_rng(seed)
    s = rng.integers(-3, 4, size=(B, V)).astype(np.float32)          # seven values: heavy ties
    if kind == "zeros":
        s[:] = 0.0
    elif kind == "special":
        s[s == 0] = np.where(rng.random((s == 0).sum()) < 0.5, -0.0, 0.0).astype(np.float32)
        s[rng.random((B, V)) < 0.1] = np.nan
        s[rng.random((B, V)) < 0.05] = np.inf
        s[rng.random((B, V)) < 0.05] = -np.inf
        s[1] = np.nan
        s[2] = -1.0                                                  # all negative: the seen zeros win
    answers = rng.integers(0, V, size=B)
    seen = []
    for b in range(B):
        row = rng.integers(0, V, size=int(rng.integers(0, 2 * V))).tolist()       # duplicates included
        row += [-1] * 3 + [V, V + 7, -5]                                          # pads and ids outside the catalogue
        if b % 3 == 0:
            row += [int(answers[b])] * 2                                          # the answer itself is seen
        seen.append(row)
    return s, seen, answers


@pytest.mark.parametrize("kind", ["ties", "zeros", "special"])
@pytest.mark.parametrize("V", [1, 2, 37, 300])
def test_reference_rank_is_the_index_in_the_full_list(kind, V):
    s, seen, answers = _case(kind, 12, V, seed=V + len(kind))
    rank, val = A.ranks(s, seen, answers)
    np.testing.assert_array_equal(rank, A.index_in_full_list(s, seen, answers))
    m = R.masked(s, seen)
    np.testing.assert_array_equal(val.view(np.uint32), m[np.arange(12), answers].view(np.uint32))
    if kind == "zeros":
        np.testing.assert_array_equal(rank, answers)                 # all ties: the column order
    # an answer outside the catalogue: -1 and NaN
    rank, val = A.ranks(s, seen, np.array([-1, V] + [0] * 10))
    assert (rank[:2] == -1).all() and np.isnan(val[:2]).all() and (rank[2:] >= 0).all()


@pytest.mark.parametrize("kind", ["ties", "special"])
@pytest.mark.parametrize("bounds", [[(0, 61)], [(0, 30), (30, 61)], [(0, 1), (1, 60), (60, 61)], [(0, 25), (25, 26), (26, 61)]])
def test_ranks_of_contiguous_parts_sum_to_the_whole(kind, bounds):
    s, seen, answers = _case(kind, 12, 61, seed=len(bounds))
    whole, val = A.ranks(s, seen, answers)
    score = np.zeros(12, np.float32)
    for lo, hi in bounds:
        part = np.zeros(12, np.float32)
        A.answer_scores(s, seen, answers, lo, hi, out=part)
        score = score + part                                          # what the all-reduce does
    np.testing.assert_array_equal(A.order_key(score), A.order_key(val))
    total = np.zeros(12, np.int64)
    for lo, hi in bounds:
        r, v = A.ranks(s, seen, answers, lo, hi, answer_score=score)
        assert (r >= 0).all()
        total += r
    np.testing.assert_array_equal(total, whole)
    # without a given score a part ranks the answers it owns and refuses the others
    for lo, hi in bounds:
        r, v = A.ranks(s, seen, answers, lo, hi)
        own = (answers >= lo) & (answers < hi)
        assert (r[~own] == -1).all() and np.isnan(v[~own]).all() and (r[own] >= 0).all()


def test_metrics_from_ranks_equal_those_from_the_hit_matrix_and_mrr():
    from bsarec_amd import ranking
    rng = np.random.default_rng(3)
    n, V = 500, 60
    s = rng.standard_normal((n, V)).astype(np.float32)
    answers = rng.integers(0, V, size=n)
    ids, _ = R.topk(s, [[]] * n, V)
    rank, _ = A.ranks(s, [[]] * n, answers)
    ks = (5, 10, 20, 1, 33, 60)
    hit = torch.from_numpy(ids == answers[:, None])
    from_hit = ranking.cutoff_metrics(ks, hit=hit)
    from_rank = ranking.cutoff_metrics(ks, ranks=rank)
    np.testing.assert_allclose(from_rank, from_hit, rtol=0, atol=1e-12)
    assert from_rank[-2] == 1.0                                       # HR@V
    assert ranking.mrr([0, 1, 3]) == pytest.approx((1 + 0.5 + 0.25) / 3, abs=1e-15)
    assert ranking.mrr(rank) == pytest.approx(float(np.mean(1.0 / (rank.astype(np.float64) + 1.0))), abs=1e-15)


def test_get_rank_score_values_and_log_line():
    from bsarec_amd.trainer import Trainer, _NullLogger
    from bsarec_amd import ranking
    tr = object.__new__(Trainer)
    tr.args, tr.logger = argparse.Namespace(item_size=100, extra_ks=()), _NullLogger()
    ranks = np.array([0, 4, 5, 19, 20, 99], np.int32)
    vals, line = tr.get_rank_score(7, ranks)
    assert len(vals) == 7
    np.testing.assert_allclose(vals[:6], ranking.cutoff_metrics((5, 10, 20), ranks=ranks), rtol=0, atol=0)
    assert vals[0] == 2 / 6 and vals[2] == 3 / 6 and vals[4] == 4 / 6
    assert vals[6] == pytest.approx(np.mean([1, 1 / 5, 1 / 6, 1 / 20, 1 / 21, 1 / 100]), abs=1e-15)
    assert line.startswith("{'Epoch': 7, 'HR@5': '0.3333'") and line.endswith(f"'MRR': '{vals[6]:.4f}'}}")
    vals, line = tr.get_rank_score(7, ranks, extra_ks=(50, 100))      # deeper than any list
    assert len(vals) == 11 and vals[6] == 5 / 6 and vals[8] == 1.0 and "'NDCG@100'" in line and line.endswith("'}")
    assert list(eval(line))[-1] == "MRR"
    with pytest.raises(ValueError, match="extra cutoffs"):
        tr.get_rank_score(7, ranks, extra_ks=(101,))
    with pytest.raises(ValueError, match="outside"):
        tr.get_rank_score(7, np.array([3, -1]))


def test_rank_is_a_full_rank_mode_and_a_cli_choice():
    from bsarec_amd.main import parse_args
    from bsarec_amd.ranking import EVAL_FULL_RANK, eval_full_rank_of
    assert EVAL_FULL_RANK == ("dense", "fused", "rank")
    assert eval_full_rank_of(argparse.Namespace(), "rank") == "rank"
    assert eval_full_rank_of(argparse.Namespace(eval_full_rank="rank")) == "rank"
    assert eval_full_rank_of(argparse.Namespace(eval_full_rank="rank"), "dense") == "dense"
    assert parse_args(["--eval_full_rank", "rank"]).eval_full_rank == "rank"
    assert parse_args(["--eval_full_rank", "rank", "--extra_ks", "50,100"]).extra_ks == (50, 100)
    with pytest.raises(SystemExit):
        parse_args(["--eval_full_rank", "rank", "--eval_negatives", "100"])


def test_sharded_topk_refuses_the_rank_mode():
    from bsarec_amd.catalogue import ShardedCatalogue
    sc = object.__new__(ShardedCatalogue)
    sc.args = argparse.Namespace()
    with pytest.raises(ValueError, match="topk: eval_full_rank = 'rank' produces no lists"):
        sc.topk(None, 20, full_rank="rank")
    sc.args = argparse.Namespace(eval_full_rank="rank")
    with pytest.raises(ValueError, match=r"use full_sort_scores\(full_rank='rank'\)"):
        sc.topk(None, 20)
    from test_shard_full_rank_cpu import _ns
    with pytest.raises(ValueError, match="runs on the GPU only"):     # the constructor takes the flag and reaches the device check
        ShardedCatalogue(_ns(eval_full_rank="rank"), 32, None, "cpu")


# ---- argument checks ---------------------------------------------------------------------------------------------------
RANK = ["h", "ldh", "item_rows", "B", "Vs", "d", "users", "indptr", "indices", "answers", "rank_out", "score_out", "stream"]
RANGE = ["h", "ldh", "item_rows", "B", "Vs", "col_base", "d", "users", "indptr", "indices", "answers", "answer_score", "rank_out",
         "score_out", "stream"]
SCORE = ["h", "ldh", "item_rows", "B", "Vs", "col_base", "d", "users", "indptr", "indices", "answers", "score_out", "stream"]
ENTRY = {"bsarec_answer_rank": RANK, "bsarec_answer_rank_range": RANGE, "bsarec_answer_score_range": SCORE}


def _valid_call():
    buf = (C.c_byte * 4096)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16       # a 16-byte aligned host address (never dereferenced)
    return buf, dict(h=p, ldh=64, item_rows=p, B=4, Vs=100, col_base=300, d=64, users=p, indptr=None, indices=None, answers=p,
                     answer_score=None, rank_out=p, score_out=p, stream=None)


COMMON = [dict(B=0), dict(B=-3), dict(Vs=0), dict(Vs=-1), dict(d=0), dict(d=2), dict(d=260), dict(d=66), dict(ldh=32), dict(h=None),
          dict(item_rows=None), dict(answers=None), dict(indptr="p"), dict(indptr="p", users=None), dict(indptr="p", indices=None),
          dict(item_rows="p+4"), dict(h="p+4")]
OF_RANGE = [dict(col_base=-1), dict(col_base=2**31 - 100), dict(col_base=2**31 - 1), dict(col_base=2**40),
            dict(Vs=2**31 - 1, col_base=1)]
CASES = ([(n, c) for n in ENTRY for c in COMMON] +
         [(n, c) for n in ("bsarec_answer_rank_range", "bsarec_answer_score_range") for c in OF_RANGE] +
         [("bsarec_answer_rank", dict(rank_out=None)), ("bsarec_answer_rank_range", dict(rank_out=None)),
          ("bsarec_answer_score_range", dict(score_out=None))])


@pytest.mark.parametrize("name,change", CASES, ids=[f"{n[7:]}-{'-'.join(f'{k}={v}' for k, v in c.items())}" for n, c in CASES])
def test_invalid_arguments_return_negative_without_a_gpu(name, change):
    from bsarec_amd import _lib
    lib = _lib.load()
    assert name in _lib.EXPORTS
    buf, kw = _valid_call()
    p = kw["h"]
    for k, v in change.items():
        kw[k] = {"p": p, "p+4": p + 4}.get(v, v) if isinstance(v, str) else v
    assert getattr(lib, name)(*[kw[k] for k in ENTRY[name]]) < 0
