"""Sampled-candidate evaluation on the host (no GPU): the numpy restatement of the protocol against the oracle's Philox, the
metric arithmetic, data.item_popularity, the command-line flags, the host-side pool check, and the C entry point's symbol,
ABI version and argument checks (which return < 0 before any HIP call)."""
import ctypes as C
import os
import shutil
import subprocess
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import sampled_eval_ref as R
from conftest import ROOT
from oracle.bsarec_oracle import philox4x32_10


# ---- the restatement ---------------------------------------------------------------------------------------------------------
def test_uniform_draws_follow_the_oracle_philox():
    user, tag, seed, V = (7 << 32) | 12345, 2, 0xDEADBEEF12345678, 3417
    items = R.draw_items(user, tag, seed, V, 5, 3)
    for i, j in enumerate(range(5, 8)):
        w = philox4x32_10(np.array([j], np.uint32), 12345, 7, tag, seed & 0xFFFFFFFF, seed >> 32)
        for m in range(4):
            assert items[4 * i + m] == 1 + (int(w[m][0]) * (V - 1) >> 32)
    assert items.min() >= 1 and items.max() <= V - 1


def test_popularity_draws_follow_the_oracle_philox():
    rng = np.random.default_rng(0)
    pop = rng.integers(0, 5, size=97).astype(np.int64)
    pop[0] = 0
    cum = np.cumsum(pop)
    T = int(cum[-1])
    user, tag, seed = 99, 1, 42
    items = R.draw_items(user, tag, seed, 97, 0, 50, cum)
    for j in range(50):
        w = [int(x[0]) for x in philox4x32_10(np.array([j], np.uint32), 99, 0, tag, 42, 0)]
        for m in range(2):
            x = w[2 * m] | (w[2 * m + 1] << 32)
            r = (x * T) >> 64
            want = next(i for i in range(97) if cum[i] > r)
            assert items[2 * j + m] == want
    assert np.all(pop[items] > 0)                        # items of count 0 are never drawn


def test_mulhi64_matches_python_integers():
    rng = np.random.default_rng(1)
    x = rng.integers(0, 2**63, size=200, dtype=np.uint64) * np.uint64(2) + np.uint64(1)
    for t in (1, 3, 2**32 - 1, 2**32 + 7, 2**62 + 12345, 2**63 - 1):
        got = R.mulhi64(x, t)
        assert [int(g) for g in got] == [(int(v) * t) >> 64 for v in x]


def test_candidates_follow_the_acceptance_rule():
    V, n = 60, 30
    seen = np.array([2, 3, 5, 8, 13, 21, 34, 55])
    answer = 13                                           # a seen answer stays the positive
    c = R.candidates(11, answer, seen, 5, 1, V, n)
    assert c[0] == answer and len(c) == n + 1
    neg = c[1:]
    assert len(set(neg.tolist())) == n and not np.isin(neg, seen).any() and answer not in neg and neg.min() >= 1
    # acceptance order = first occurrence among the eligible draws of the stream
    d = R.draw_items(11, 1, 5, V, 0, 256)
    order = []
    for it in d:
        if it != answer and it not in seen and it not in order:
            order.append(int(it))
    assert neg.tolist() == order[:n]
    # a different tag or seed gives a different stream
    assert not np.array_equal(R.candidates(11, answer, seen, 5, 2, V, n), c)
    assert not np.array_equal(R.candidates(11, answer, seen, 6, 1, V, n), c)


def test_exactly_n_eligible_and_too_few():
    V = 40
    seen = np.arange(1, 20)
    n = R.eligible_count(30, seen, V)
    assert n == 19                                        # 20..39 without 30
    c = R.candidates(3, 30, seen, 1, 1, V, n)
    assert sorted(c[1:].tolist()) == sorted(set(range(20, 40)) - {30})
    assert R.candidates(3, 30, seen, 1, 1, V, n + 1) is None


def test_rank_and_metric_arithmetic():
    assert R.rank_of([1.0, 0.5, 2.0, 1.0, np.nan]) == 3   # above, equal and NaN count against the model
    assert R.rank_of([np.nan, 0.0, 1.0]) == 2
    assert R.rank_of([np.inf, np.inf, 1.0]) == 1
    ranks = np.array([0, 4, 5, 9, 19, 20, 100])
    got = R.metrics(ranks)
    want = []
    for k in (5, 10, 20):
        want += [sum(r < k for r in ranks) / 7, sum(1 / np.log2(r + 2) for r in ranks if r < k) / 7]
    np.testing.assert_allclose(got, want, rtol=1e-15)
    from bsarec_amd.trainer import sampled_metrics
    for k in (1, 5, 10, 20, 101):
        np.testing.assert_allclose(sampled_metrics(ranks, k), R.metrics(ranks, (k,)), rtol=1e-15)


# ---- data / CLI / trainer host logic -------------------------------------------------------------------------------------------
def test_item_popularity_counts_the_training_part():
    from bsarec_amd.data import item_popularity
    seqs = [[1, 2, 2, 3, 4], [3, 3, 5], [6, 7], [1]]
    got = item_popularity(seqs, 9)
    # training parts s[:-2]: [1, 2, 2], [3], [], []
    assert got.dtype == np.int64 and got.tolist() == [0, 1, 2, 1, 0, 0, 0, 0, 0]


def test_eval_flags_parse():
    from bsarec_amd.main import parse_args
    from bsarec_amd.trainer import sampled_protocol
    a = parse_args([])
    assert not hasattr(a, "eval_negatives") and not hasattr(a, "eval_sampler") and not hasattr(a, "eval_seed")
    assert sampled_protocol(a) == (0, "uniform", 42)
    a = parse_args(["--eval_negatives", "100", "--eval_sampler", "popularity", "--eval_seed", "7"])
    assert (a.eval_negatives, a.eval_sampler, a.eval_seed) == (100, "popularity", 7)
    assert sampled_protocol(a) == (100, "popularity", 7)
    assert sampled_protocol(parse_args(["--eval_negatives", "1024", "--seed", "3"])) == (1024, "uniform", 3)
    assert parse_args(["--eval_negatives", "0"]).eval_negatives == 0
    assert parse_args(["--eval_seed", str(2**64 - 1)]).eval_seed == 2**64 - 1
    assert parse_args(["--eval_negatives", "100", "--extra_ks", "50,101"]).extra_ks == (50, 101)


@pytest.mark.parametrize("bad", [["--eval_negatives", "-1"], ["--eval_negatives", "1025"], ["--eval_negatives", "x"],
                                 ["--eval_sampler", "zipf"], ["--eval_seed", "-1"], ["--eval_seed", str(2**64)],
                                 ["--eval_negatives", "100", "--extra_ks", "102"]])
def test_eval_flags_reject(bad):
    from bsarec_amd.main import parse_args
    with pytest.raises(SystemExit):
        parse_args(bad)


def _fake_trainer(**kw):
    import scipy.sparse as sp
    from bsarec_amd.ranking import sampling_tables
    seen = [[1, 2, 3], [], [4, 5, 6, 7, 8, 9]]
    indptr = np.concatenate([[0], np.cumsum([len(s) for s in seen])])
    mat = sp.csr_matrix((np.ones(indptr[-1]), np.concatenate(seen).astype(np.int64), indptr), shape=(3, 12))
    args = types.SimpleNamespace(train_matrix=mat, item_size=12, seed=1, **kw)
    logs = []
    fake = types.SimpleNamespace(args=args, device=torch.device("cpu"), logger=types.SimpleNamespace(info=logs.append))
    fake._sampling_tables = lambda sampler, V: sampling_tables(mat, sampler, getattr(args, "item_popularity", None), V, fake.device)
    return fake, logs, seen


def test_host_pool_check_names_the_short_users():
    from bsarec_amd.ranking import check_pool
    fake, _, seen = _fake_trainer()
    t = fake._sampling_tables("uniform", 12)
    users, answers = np.array([0, 1, 2]), np.array([3, 10, 11])
    for u, a in zip(users, answers):                      # the host count agrees with the restatement's
        assert t["pool"] - t["seen_w"][u] - (0 if a in seen[u] else t["w"][a]) == R.eligible_count(a, seen[u], 12)
    check_pool(t, users, answers, 4, 12)          # eligible: 8, 10, 4
    with pytest.raises(ValueError, match=r"users \[2\]"):
        check_pool(t, users, answers, 5, 12)
    with pytest.raises(ValueError, match="outside"):
        check_pool(t, users, np.array([3, 0, 11]), 1, 12)
    pop = np.array([0, 5, 0, 1, 1, 1, 1, 1, 1, 1, 0, 2])   # drawable: 1, 3..9, 11
    fake, _, _ = _fake_trainer(item_popularity=pop)
    t = fake._sampling_tables("popularity", 12)
    assert t["cum"].tolist() == np.cumsum(pop).tolist()
    for u, a in zip(users, answers):
        assert t["pool"] - t["seen_w"][u] - (0 if a in seen[u] else t["w"][a]) == R.eligible_count(a, seen[u], 12, pop)
    check_pool(t, users, answers, 2, 12)
    with pytest.raises(ValueError, match=r"users \[2\]"):   # user 2: 1, 3 and 11 left, answer 11 -> 2
        check_pool(t, users, answers, 3, 12)


def test_get_sampled_score_positions_and_protocol_key():
    from bsarec_amd.main import monitored_score
    from bsarec_amd.trainer import Trainer
    fake, logs, _ = _fake_trainer(eval_negatives=100, eval_sampler="popularity")
    ranks = np.array([0, 3, 7, 12, 50, 100])
    scores, txt = Trainer.get_sampled_score(fake, 4, torch.as_tensor(ranks, dtype=torch.int32))
    np.testing.assert_allclose(scores, R.metrics(ranks), rtol=1e-15)
    assert monitored_score(scores).tolist() == [scores[5]]
    assert list(logs[0]) == ["Epoch", "HR@5", "NDCG@5", "HR@10", "NDCG@10", "HR@20", "NDCG@20", "Protocol"]
    assert logs[0]["Protocol"] == "popularity-100" and logs[0]["Epoch"] == 4
    fake.args.extra_ks = (50, 101)
    scores, _ = Trainer.get_sampled_score(fake, 0, ranks)
    np.testing.assert_allclose(scores, R.metrics(ranks, (5, 10, 20, 50, 101)), rtol=1e-15)
    with pytest.raises(ValueError):
        Trainer.get_sampled_score(fake, 0, ranks, extra_ks=(102,))
    with pytest.raises(ValueError):
        Trainer.get_sampled_score(fake, 0, np.array([1, -1]))


# ---- the C entry point -----------------------------------------------------------------------------------------------------------
def test_library_exports_sampled_rank_at_abi_10():
    from bsarec_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 10 and lib.bsarec_abi_version() == 10
    assert hasattr(lib, "bsarec_sampled_rank")
    assert (_lib.NEG_MAX, _lib.NEG_MAX_DRAWS) == (1024, 1 << 20)
    header = open(os.path.join(ROOT, "include", "bsarec_hip.h")).read()
    assert "#define BSAREC_NEG_MAX 1024" in header and "#define BSAREC_NEG_MAX_DRAWS (1 << 20)" in header


def _valid_call():
    buf = (C.c_byte * 4096)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16       # a 16-byte aligned host address (never dereferenced)
    return buf, dict(h=p, ldh=64, item_emb=p, B=4, V=100, d=64, users=p, answers=p, indptr=None, indices=None, pop_cum=None,
                     n_neg=10, seed=1, tag=1, rank_out=p, cand_out=None, score_out=None, stream=None)


ORDER = ["h", "ldh", "item_emb", "B", "V", "d", "users", "answers", "indptr", "indices", "pop_cum", "n_neg", "seed", "tag",
         "rank_out", "cand_out", "score_out", "stream"]


@pytest.mark.parametrize("change", [dict(n_neg=0), dict(n_neg=1025), dict(V=1), dict(V=0), dict(d=2), dict(d=260),
                                    dict(d=66), dict(ldh=32), dict(B=0), dict(h=None), dict(item_emb=None), dict(users=None),
                                    dict(answers=None), dict(rank_out=None), dict(indptr="p"), dict(item_emb="p+4")])
def test_invalid_arguments_return_negative_without_a_gpu(change):
    from bsarec_amd import _lib
    lib = _lib.load()
    buf, kw = _valid_call()
    p = kw["h"]
    for k, v in change.items():
        kw[k] = {"p": p, "p+4": p + 4}.get(v, v) if isinstance(v, str) else v
    assert lib.bsarec_sampled_rank(*[kw[k] for k in ORDER]) < 0


def test_header_declares_sampled_rank_for_c99(tmp_path):
    """A C99 program that includes the header compiles, links against the library and gets < 0 from an invalid call."""
    lib_dir = os.path.join(ROOT, "bsarec_amd")
    if not os.path.exists(os.path.join(lib_dir, "libbsarec_hip.so")) or not shutil.which("gcc"):
        pytest.skip("library or gcc missing")
    src = r"""
#include "bsarec_hip.h"
#include <stdio.h>
int main(void) {
    static float h[64], e[64 * 4];
    int64_t users[1] = {0}, answers[1] = {1};
    int32_t rank[1];
    int bad_n = bsarec_sampled_rank(h, 64, e, 1, 4, 64, users, answers, NULL, NULL, NULL, BSAREC_NEG_MAX + 1, 7u, 1u, rank,
                                    NULL, NULL, NULL);
    int bad_v = bsarec_sampled_rank(h, 64, e, 1, 1, 64, users, answers, NULL, NULL, NULL, 1, 7u, 1u, rank, NULL, NULL, NULL);
    printf("%d %d %d %d\n", bsarec_abi_version(), BSAREC_NEG_MAX_DRAWS, bad_n, bad_v);
    return (bad_n < 0 && bad_v < 0) ? 0 : 1;
}
"""
    f = tmp_path / "host.c"
    f.write_text(src)
    exe = tmp_path / "host"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(f), "-o", str(exe),
                    "-L", lib_dir, "-lbsarec_hip", f"-Wl,-rpath,{lib_dir}"], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ver, draws, _, _ = r.stdout.split()
    assert int(ver) == 10 and int(draws) == 1 << 20
