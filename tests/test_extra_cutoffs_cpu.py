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


def test_rank_operand_returns_itself_or_an_aligned_fp32_copy():
    from bsarec_amd.ranking import rank_operand
    good = torch.randn(8, 8)
    assert good.data_ptr() % 16 == 0 and rank_operand(good) is good
    padded = torch.randn(8, 12)[:, :8]                    # row stride 12: still a multiple of 4
    assert rank_operand(padded) is padded
    shifted = torch.randn(8 * 8 + 1)[1:].view(8, 8)       # one element past a 16-byte boundary
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    for bad in (torch.randn(8, 8).bfloat16(), torch.randn(8, 16)[:, ::2], shifted, torch.randn(8, 6)[:, :4]):
        out = rank_operand(bad)
        assert out is not bad and out.dtype == torch.float32 and out.is_contiguous() and out.data_ptr() % 16 == 0
        assert out.shape == bad.shape and torch.equal(out, bad.float())


def test_cutoff_metrics_and_post_fix_key_order():
    import types
    from bsarec_amd.ranking import cutoff_metrics, metrics_post_fix
    from bsarec_amd.trainer import Trainer
    pos = [0, 7, 19, None]                                # the answer's place in each of the 4 lists; None: not in the list
    hit = torch.zeros(4, 25, dtype=torch.bool)
    for row, p in enumerate(pos):
        if p is not None:
            hit[row, p] = True
    ks = (5, 10, 20, 25)
    want = []
    for k in ks:
        at = [p for p in pos if p is not None and p < k]
        want += [len(at) / 4, sum(1.0 / np.log2(p + 2.0) for p in at) / 4]
    assert want[:2] == [0.25, 0.25] and want[6] == 0.75
    got = cutoff_metrics(ks, hit=hit)
    np.testing.assert_allclose(got, want, rtol=1e-14, atol=0)        # float64 throughout: a few roundings
    np.testing.assert_allclose(cutoff_metrics(ks, ranks=[0, 7, 19, 25]), want, rtol=1e-14, atol=0)
    keys = ["Epoch", "HR@5", "NDCG@5", "HR@10", "NDCG@10", "HR@20", "NDCG@20", "HR@25", "NDCG@25"]
    full = metrics_post_fix(3, ks, got)
    assert list(full) == keys and full["Epoch"] == 3
    assert [full[k] for k in keys[1:]] == ['{:.4f}'.format(v) for v in want]
    sampled = metrics_post_fix(3, ks, got, protocol="uniform-100")
    assert list(sampled) == keys + ["Protocol"] and sampled["Protocol"] == "uniform-100"
    # the reporters: the reference's six values first, then the extra cutoffs; the same keys in the same order
    logs = []
    fake = types.SimpleNamespace(args=types.SimpleNamespace(extra_ks=(25,), eval_negatives=100, seed=1), device=torch.device("cpu"),
                                 logger=types.SimpleNamespace(info=logs.append))
    answers = torch.arange(1, 5)
    pred = torch.zeros(4, 25, dtype=torch.int64)
    pred[hit] = answers[:3]
    scores, txt = Trainer.get_full_sort_score(fake, 3, answers, pred)
    np.testing.assert_allclose(scores, want, rtol=1e-14, atol=0)
    assert list(logs[0]) == keys and txt == str(full)
    scores, txt = Trainer.get_sampled_score(fake, 3, torch.tensor([0, 7, 19, 25]))
    np.testing.assert_allclose(scores, want, rtol=1e-14, atol=0)
    assert list(logs[1]) == keys + ["Protocol"] and txt == str(sampled)
