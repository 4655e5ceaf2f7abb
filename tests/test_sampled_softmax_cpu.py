"""The sampled-softmax training head on the host: flag parsing, the refusals raised before a GPU is needed, and the numpy
restatement (tests/sampled_softmax_ref.py) against finite differences in float64."""
import argparse

import numpy as np
import pytest

import sampled_softmax_ref as R


def _args(**kw):
    a = argparse.Namespace(item_size=97, hidden_size=16, max_seq_length=8, batch_size=4, hidden_dropout_prob=0.0,
                           attention_probs_dropout_prob=0.0, num_hidden_layers=1, num_attention_heads=1, hidden_act="gelu",
                           initializer_range=0.02, c=3, alpha=0.9, seed=42)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_flags_ranges_and_suppress():
    from bsarec_amd import main as M
    a = M.parse_args([])
    for k in ("train_negatives", "train_sampler", "train_no_logq"):
        assert not hasattr(a, k)
    a = M.parse_args(["--train_negatives", "8192", "--train_sampler", "popularity", "--train_no_logq"])
    assert (a.train_negatives, a.train_sampler, a.train_no_logq) == (8192, "popularity", True)
    assert M.parse_args(["--train_negatives", "0"]).train_negatives == 0
    for bad in (["--train_negatives", "8193"], ["--train_negatives", "-1"], ["--train_negatives", "x"],
                ["--train_sampler", "zipf"]):
        with pytest.raises(SystemExit):
            M.parse_args(bad)


def test_train_head_of_args():
    from bsarec_amd import _lib as Lb
    from bsarec_amd.model import train_head_of
    assert train_head_of(_args()) == {"train_negatives": 0, "train_sampler": 0, "train_no_logq": 0}
    assert train_head_of(_args(train_negatives=5, train_sampler="popularity", train_no_logq=True)) == \
        {"train_negatives": 5, "train_sampler": 1, "train_no_logq": 1}
    with pytest.raises(ValueError):
        train_head_of(_args(train_negatives=Lb.TRAIN_NEG_MAX + 1))
    with pytest.raises(ValueError):
        train_head_of(_args(train_negatives=4, train_sampler="zipf"))
    assert Lb.Config.train_negatives.offset > Lb.Config.x3_products.offset        # the tail of bsarec_config_t


@pytest.mark.parametrize("name", ["SASRecModel", "FMLPRecModel", "DuoRecModel"])
def test_sibling_models_refuse_a_sampled_head(name):
    from bsarec_amd import model as Mo
    with pytest.raises(ValueError, match="train_negatives"):
        getattr(Mo, name)(_args(train_negatives=16, tau=1.0, lmd=0.1, lmd_sem=0.1, ssl="us_x", sim="dot"))


def test_bsarec_model_refuses_bf16_with_a_sampled_head():
    from bsarec_amd import BSARecModel
    with pytest.raises(ValueError, match="fp32"):
        BSARecModel(_args(train_negatives=16, storage="bf16"))
    BSARecModel(_args(train_negatives=16))                  # fp32: accepted (no GPU needed to construct)


class _FakeModel:
    def __init__(self, n, sampler):
        self.train_head = {"train_negatives": n, "train_sampler": sampler, "train_no_logq": 0}
        self.table = None

    def set_train_popularity(self, pop):
        self.table = pop


class _FakeLoader:
    def __init__(self, answers):
        self.answers = np.asarray(answers, dtype=np.int64)


def test_trainer_checks_before_the_first_step():
    from bsarec_amd.trainer import check_train_head
    pop = np.array([0, 3, 0, 5, 1], dtype=np.int64)
    check_train_head(_FakeModel(0, 0), _args(), _FakeLoader([2]), process_group=object())      # full CE: nothing to check
    with pytest.raises(ValueError, match="data-parallel"):
        check_train_head(_FakeModel(8, 0), _args(), _FakeLoader([1]), process_group=object())
    with pytest.raises(ValueError, match="item_popularity"):
        check_train_head(_FakeModel(8, 1), _args(), _FakeLoader([1]))
    with pytest.raises(ValueError, match="2 training answers"):
        check_train_head(_FakeModel(8, 1), _args(item_popularity=pop), _FakeLoader([1, 2, 3, 2, 4]))
    m = _FakeModel(8, 1)
    check_train_head(m, _args(item_popularity=pop), _FakeLoader([1, 3, 4]))
    assert m.table is not None
    m = _FakeModel(8, 0)
    check_train_head(m, _args(), _FakeLoader([1, 2]))                 # uniform: no table
    assert m.table is None


def test_sharded_catalogue_refuses():
    from bsarec_amd.catalogue import ShardedCatalogue
    with pytest.raises(ValueError, match="train_negatives"):
        ShardedCatalogue(_args(train_negatives=64), 4, None, "cpu")


def test_draws_follow_the_stream_layout():
    V, N = 1000, 11
    d = R.draws(7, 3, V, N)
    assert d.shape == (N,) and ((d >= 1) & (d < V)).all()
    assert np.array_equal(R.draws(7, 3, V, 8), d[:8])                 # a prefix of the same stream
    assert not np.array_equal(R.draws(7, 4, V, N), d)
    counts = np.array([0, 0, 4, 0, 1, 9], dtype=np.int64)
    cum = R.cumulative(counts)
    p = R.draws(7, 3, 6, 4000, cum)
    assert set(np.unique(p)) <= {2, 4, 5}
    freq = np.bincount(p, minlength=6)[[2, 4, 5]] / 4000
    assert np.abs(freq - np.array([4, 1, 9]) / 14).max() < 0.03
    c = R.corrections(np.array([2, 5]), 10, cum)
    np.testing.assert_allclose(c, np.log(10 * np.array([4, 9]) / 14))
    assert (R.corrections(np.array([2, 5]), 10, cum, logq=False) == 0).all()


@pytest.mark.parametrize("pop", [False, True])
def test_restated_head_against_finite_differences(pop):
    rng = np.random.default_rng(1)
    V, d, B, N = 9, 5, 4, 12
    h = rng.standard_normal((B, d))
    E = rng.standard_normal((V, d))
    counts = np.array([0, 2, 1, 3, 1, 4, 2, 1, 5]) if pop else None
    cum = R.cumulative(counts) if pop else None
    cand = R.draws(3, 1, V, N, cum)
    ans = np.array([1, cand[0], 5, 8])                    # row 1 hits the first candidate
    loss, dh, dE = R.grads(h, E, ans, cand, cum)
    x, _, _, g = R.head(h, E, ans, cand, cum)
    assert np.isinf(x[1, 1]) and g[1, 1] == 0 and np.isfinite(loss)
    eps = 1e-6
    for arr, grad in ((h, dh), (E, dE)):
        num = np.zeros_like(arr)
        for idx in np.ndindex(arr.shape):
            old = arr[idx]
            arr[idx] = old + eps
            lp = R.head(h, E, ans, cand, cum)[2]
            arr[idx] = old - eps
            lm = R.head(h, E, ans, cand, cum)[2]
            arr[idx] = old
            num[idx] = (lp - lm) / (2 * eps)
        np.testing.assert_allclose(grad, num, rtol=1e-6, atol=1e-8)
    unused = np.setdiff1d(np.arange(V), np.concatenate([ans, cand]))
    assert (dE[unused] == 0).all()
