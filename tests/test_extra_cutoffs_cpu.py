"""--extra_ks (evaluation cutoffs beyond the reference's 5 / 10 / 20) on the host: parsing, and early stopping that keeps
monitoring NDCG@20 when extra values follow it."""
import logging

import numpy as np
import pytest

torch = pytest.importorskip("torch")


def test_extra_ks_default_is_none():
    from bsarec_amd.main import parse_args
    assert tuple(parse_args([]).extra_ks) == ()


def test_extra_ks_parses_a_comma_list():
    from bsarec_amd.main import parse_args
    assert parse_args(["--extra_ks", "50,100"]).extra_ks == (50, 100)
    assert parse_args(["--extra_ks", "1024"]).extra_ks == (1024,)
    assert parse_args(["--extra_ks", "100, 50,100"]).extra_ks == (100, 50)
    assert parse_args(["--extra_ks", ""]).extra_ks == ()


@pytest.mark.parametrize("bad", ["0", "1025", "-5", "50,abc", "2000,50"])
def test_extra_ks_rejects_values_outside_1_to_1024(bad):
    from bsarec_amd.main import parse_args
    with pytest.raises(SystemExit):
        parse_args(["--extra_ks", bad])


def test_early_stopping_monitors_ndcg20_with_extra_cutoffs():
    from bsarec_amd.main import EarlyStopping, monitored_score
    six = [0.1, 0.2, 0.3, 0.4, 0.5, 0.6]
    assert monitored_score(six).tolist() == [0.6]
    assert monitored_score(six + [0.7, 0.8, 0.9, 0.95]).tolist() == [0.6]

    model = torch.nn.Linear(2, 2)
    stop = EarlyStopping(None, logging.getLogger("test_extra_cutoffs"), patience=2)
    # NDCG@20 falls while the extra cutoffs' values rise: the counter must run out
    for i, nd20 in enumerate((0.5, 0.4, 0.3)):
        stop(monitored_score([0.0] * 5 + [nd20] + [0.1 * i, 0.2 * i, 0.3 * i, 0.4 * i]), model)
    assert stop.early_stop and stop.best_score.tolist() == [0.5]
    assert np.array_equal(stop.best_score, np.array([0.5]))
