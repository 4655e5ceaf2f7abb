"""Lazy (sparse) Adam for the item table on the host: the flag, the refusals raised before a GPU is needed, the C layout of
the new config field, and a self-check of the numpy restatement (tests/lazy_adam_ref.py)."""
import argparse
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import lazy_adam_ref as R


def _args(**kw):
    a = argparse.Namespace(item_size=97, hidden_size=16, max_seq_length=8, batch_size=4, hidden_dropout_prob=0.0,
                           attention_probs_dropout_prob=0.0, num_hidden_layers=1, num_attention_heads=1, hidden_act="gelu",
                           initializer_range=0.02, c=3, alpha=0.9, seed=42)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_flag_parsing_and_suppress():
    from bsarec_amd import main as M
    assert not hasattr(M.parse_args([]), "train_lazy_adam")
    assert not hasattr(M.parse_args(["--train_negatives", "64"]), "train_lazy_adam")
    a = M.parse_args(["--train_negatives", "64", "--train_lazy_adam"])
    assert a.train_lazy_adam is True and a.train_negatives == 64


def test_model_reads_the_flag():
    from bsarec_amd import BSARecModel
    assert BSARecModel(_args(train_negatives=16, train_lazy_adam=True)).lazy_adam is True
    assert BSARecModel(_args(train_negatives=16)).lazy_adam is False
    assert BSARecModel(_args()).lazy_adam is False


def test_flag_without_a_sampled_head_is_refused():
    from bsarec_amd import BSARecModel
    with pytest.raises(ValueError, match="train_negatives"):
        BSARecModel(_args(train_lazy_adam=True))
    with pytest.raises(ValueError, match="train_negatives"):
        BSARecModel(_args(train_negatives=0, train_lazy_adam=True))


@pytest.mark.parametrize("name", ["SASRecModel", "FMLPRecModel", "DuoRecModel"])
def test_sibling_models_refuse_lazy_adam(name):
    from bsarec_amd import model as Mo
    for n in (0, 16):
        with pytest.raises(ValueError, match="train_lazy_adam"):
            getattr(Mo, name)(_args(train_negatives=n, train_lazy_adam=True, tau=1.0, lmd=0.1, lmd_sem=0.1, ssl="us_x",
                                    sim="dot"))


def test_adam_step_on_a_lazy_model_is_refused():
    from bsarec_amd import BSARecModel
    m = BSARecModel(_args(train_negatives=16, train_lazy_adam=True))
    with pytest.raises(ValueError, match="lazy"):
        m.adam_step()


class _FakeModel:
    def __init__(self, lazy):
        self.train_head = {"train_negatives": 8, "train_sampler": 0, "train_no_logq": 0}
        self.lazy_adam = lazy


def test_check_train_head_refuses_a_process_group():
    from bsarec_amd.trainer import check_train_head
    with pytest.raises(ValueError, match="train_lazy_adam"):
        check_train_head(_FakeModel(True), _args(), None, process_group=object())
    check_train_head(_FakeModel(True), _args(), None)                 # single GPU, uniform sampler: nothing to refuse


def test_catalogue_sharding_refuses_the_flag():
    from bsarec_amd.catalogue import ShardedCatalogue
    with pytest.raises(ValueError, match="lazy"):
        ShardedCatalogue(_args(train_lazy_adam=True), 4, None, "cpu")


def test_train_head_fields_are_unchanged():
    from bsarec_amd import _lib as Lb
    from bsarec_amd.model import train_head_of
    assert Lb.TRAIN_FIELDS == ("train_negatives", "train_sampler", "train_no_logq")
    assert train_head_of(_args(train_negatives=5, train_lazy_adam=True)) == \
        {"train_negatives": 5, "train_sampler": 0, "train_no_logq": 0}
    assert Lb.Config.train_lazy_adam.offset > Lb.Config.train_no_logq.offset


def test_config_offset_matches_the_header(tmp_path):
    """ctypes Config.train_lazy_adam sits where the C compiler puts bsarec_config_t.train_lazy_adam, and the library refuses
    a lazy configuration without a sampled head (workspace size 0)."""
    from bsarec_amd import _lib as Lb
    from bsarec_amd import build as Bd
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    Bd.build(force=False, verbose=False)
    lib_dir = os.path.join(root, "bsarec_amd")
    src = r"""
#include "bsarec_hip.h"
#include <stddef.h>
#include <stdio.h>
int main(void) {
    bsarec_config_t cfg = {256, 50, 64, 2, 2, 3417, 2, 0.9f, 1e-12f, 0.5f, 0.5f, 0};
    cfg.train_negatives = 64;
    size_t plain = bsarec_workspace_bytes(&cfg);
    cfg.train_lazy_adam = 1;
    size_t lazy = bsarec_workspace_bytes(&cfg);
    cfg.train_negatives = 0;
    size_t bad = bsarec_workspace_bytes(&cfg);
    printf("%zu %zu %zu %zu %zu\n", offsetof(bsarec_config_t, train_lazy_adam), sizeof(bsarec_config_t), plain, lazy, bad);
    return 0;
}
"""
    f = tmp_path / "lazy.c"
    f.write_text(src)
    exe = tmp_path / "lazy"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(root, "include"), str(f), "-o", str(exe),
                    "-L", lib_dir, "-lbsarec_hip", f"-Wl,-rpath,{lib_dir}"], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    off, size, plain, lazy, bad = (int(x) for x in r.stdout.split())
    assert off == Lb.Config.train_lazy_adam.offset and size == C.sizeof(Lb.Config)
    assert plain > 0 and bad == 0
    # the marks (int32 [V]) and the list (int32 [min(V, B L + B + N)]) and the count, each carved at 256-byte granularity
    up = lambda n: -(-n // 256) * 256
    assert lazy - plain == up(4 * 3417) + up(4 * 3417) + 256


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_restatement_first_step_equals_dense_where_it_must(wd):
    rng = np.random.default_rng(1)
    V, d = 50, 8
    w = rng.standard_normal((V, d)).astype(np.float32)
    zero = np.zeros_like(w)
    ids = rng.integers(0, V, size=(3, 5))
    T = R.touched(ids, [1, 7, 7], [3, 3, 49], V)
    assert T.tolist() == sorted(set(ids[ids != 0].tolist()) | {1, 7, 3, 49})
    g = np.zeros_like(w)
    g[T] = rng.standard_normal((len(T), d)).astype(np.float32)
    g[T[0]] = 0                                                    # a touched row with an exactly zero gradient
    lw, lm, lv = R.lazy_step(w, zero, zero, g[T], T, 1, 1e-3, 0.9, 0.999, 1e-8, wd)
    dw, dm, dv = R.dense_step(w, zero, zero, g, 1, 1e-3, 0.9, 0.999, 1e-8, wd)
    out = np.setdiff1d(np.arange(V), T)
    assert (lw[out] == w[out]).all() and (lm[out] == 0).all() and (lv[out] == 0).all()
    if wd == 0:                        # from zero moments a zero gradient leaves a row as it was: one step, every row equal
        assert np.array_equal(lw, dw) and np.array_equal(lm, dm) and np.array_equal(lv, dv)
    else:                              # weight decay moves every row of the dense update, and only T under lazy Adam
        assert np.array_equal(lw[T], dw[T]) and not np.array_equal(lw[out], dw[out])
    assert not np.array_equal(lw[T], w[T])


def test_restatement_bias_corrections():
    s1, c1 = R.corrections(1, 1e-3, 0.9, 0.999)
    assert s1.dtype == np.float32 and c1.dtype == np.float32
    assert abs(float(s1) / (1e-3 / (1 - 0.9)) - 1) < 1e-5 and abs(float(c1) / np.sqrt(1 - 0.999) - 1) < 1e-4
    s5, _ = R.corrections(5, 1e-3, 0.9, 0.999)
    assert abs(float(s5) / (1e-3 / (1 - 0.9 ** 5)) - 1) < 1e-5
