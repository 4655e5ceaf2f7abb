"""Refusals of the catalogue-sharded step's head flags (bsarec_amd/catalogue.py): raised on the host before any process
group, allocation or launch is touched -- the single-GPU flags keep their limits."""
import argparse

import pytest

torch = pytest.importorskip("torch")


def _ns(**kw):
    a = argparse.Namespace(item_size=301, hidden_size=64, max_seq_length=50, batch_size=32, hidden_dropout_prob=0.0,
                           attention_probs_dropout_prob=0.0, num_hidden_layers=2, num_attention_heads=2,
                           hidden_act="gelu", initializer_range=0.02, c=3, alpha=0.9, seed=42)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw,match", [
    (dict(train_negatives=8193), "train_negatives"),
    (dict(train_negatives=-1), "train_negatives"),
    (dict(train_negatives=64, train_sampler="zipf"), "train_sampler"),
    (dict(train_lazy_adam=True), "train_lazy_adam"),
    (dict(train_negatives=0, train_lazy_adam=True), "train_lazy_adam"),
    (dict(train_negatives=64, storage="bf16"), "fp32"),
    (dict(train_negatives=64, train_lazy_adam=True, storage="bf16"), "fp32"),
])
def test_sharded_catalogue_refuses_on_the_host(kw, match):
    from bsarec_amd.catalogue import ShardedCatalogue
    with pytest.raises(ValueError, match=match):
        ShardedCatalogue(_ns(**kw), 32, None, "cpu")          # no group: the refusal comes first


def test_sampled_flags_pass_the_flag_checks():
    """N = 8192 (the limit) with every sampler option passes the flag checks: what stops it on the host is the device --
    the catalogue-sharded step runs on the GPU only."""
    from bsarec_amd.catalogue import ShardedCatalogue
    for kw in (dict(train_negatives=8192), dict(train_negatives=1, train_sampler="popularity", train_no_logq=True),
               dict(train_negatives=64, train_lazy_adam=True), dict()):
        with pytest.raises(ValueError, match="runs on the GPU only") as e:
            ShardedCatalogue(_ns(**kw), 32, None, "cpu")
        n = kw.get("train_negatives", 0)
        assert (f"train_negatives = {n}" in str(e.value)) == (n > 0), str(e.value)
