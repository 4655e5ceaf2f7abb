"""The range form of the full-catalogue CE head and the catalogue-sharded step's ``shard_ce_head`` flag on the host, no GPU:
the partition rule in fp64 (shard_ce_head_ref against ce_head_ref), the exported symbols, the workspace size, the argument
refusals of the three device entry points (they return < 0 before any HIP call), and the flag's refusals."""
import argparse
import ctypes as C
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import rel_l2
import ce_head_ref as R
import shard_ce_head_ref as SR

SYMBOLS = ("bsarec_ce_head_range_workspace_bytes", "bsarec_ce_head_range_stats", "bsarec_ce_head_range_merge",
           "bsarec_ce_head_range_bwd")


@pytest.mark.parametrize("W", [1, 2, 3, 8])
@pytest.mark.parametrize("V", [5, 37, 301, 302])
def test_partition_rule(V, W):
    """Per-range (max, sum, target) merged in rank order give the whole table's rows and loss; the ranges' dh parts add up to
    dh; a range's dE is the matching slice of the whole table's dE.  fp64, gate 1e-12."""
    Bg, d, g = 24, 12, 0.37
    rng = np.random.default_rng(1000 * V + W)
    h, E = rng.normal(0, 1, (Bg, d)), rng.normal(0, 1, (V, d))
    a = rng.integers(0, V, Bg)
    cut = SR.ranges(V, W)
    assert sum(vs for _, vs in cut) == V and all(lo + vs <= V for lo, vs in cut)
    if W == 8 and V == 5:
        assert [vs for _, vs in cut] == [1, 1, 1, 1, 1, 0, 0, 0]          # ranks that own nothing
    forced = [0, V - 1, -3, V + 5] + [x for lo, vs in cut if vs for x in (lo, lo + vs - 1)]
    a[:len(forced)] = forced[:Bg]
    want_loss, want_rows, want_dh, want_dE = R.ce_head(h, E, a, g)
    loss, rows, dh_parts, dE_parts, stats_all = SR.sharded_ce_head(h, E, a, W, g)
    for (lo, vs), st in zip(cut, stats_all):
        if vs == 0:
            assert (st[0] == -np.inf).all() and not st[1:].any()
    assert (np.count_nonzero(stats_all[:, 2], axis=0) <= 1).all()         # one owner per answer
    assert abs(loss - want_loss) <= 1e-12
    assert np.abs(rows - want_rows).max() <= 1e-12
    assert np.abs(sum(dh_parts) - want_dh).max() <= 1e-12
    for (lo, vs), dE in zip(cut, dE_parts):
        assert dE.shape == (vs, d)
        if vs:
            assert np.abs(dE - want_dE[lo:lo + vs]).max() <= 1e-12
    assert rel_l2(np.concatenate(dE_parts), want_dE) <= 1e-12


def test_symbols_are_declared_exported_and_bound():
    from bsarec_amd import _lib
    lib = _lib.load()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "bsarec_hip.h")).read()
    for name in SYMBOLS:
        assert name + "(" in header, name
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes == _lib.EXPORTS[name][1]
    assert lib.bsarec_abi_version() == 10                     # additive symbols


def test_workspace_bytes():
    from bsarec_amd import _lib
    lib = _lib.load()
    f, one = lib.bsarec_ce_head_range_workspace_bytes, lib.bsarec_ce_head_workspace_bytes
    for Bg, Vs, d in ((1, 1, 4), (33, 1000, 100), (64, 200_001, 64), (2048, 1_250_001, 256)):
        assert f(Bg, Vs, d) == one(Bg, Vs, d) > 0, (Bg, Vs, d)
    assert f(32, 0, 64) == one(32, 1, 64) > 0                 # a rank that owns nothing
    for Bg, Vs, d in ((8, 100, 66), (8, 100, 2), (8, 0, 66), (65537, 100, 64), (65537, 0, 64), (0, 100, 64), (8, -1, 64)):
        assert f(Bg, Vs, d) <= 0, (Bg, Vs, d)


STATS = ["h", "ldh", "item_rows", "Bg", "Vs", "col_base", "item_size", "d", "answers", "stats", "workspace", "workspace_bytes",
         "stream"]
MERGE = ["stats_all", "world", "Bg", "workspace", "workspace_bytes", "loss_rows", "loss", "stream"]
BWD = ["h", "ldh", "item_rows", "Bg", "Vs", "col_base", "item_size", "d", "answers", "gout", "workspace", "workspace_bytes",
       "dh_part", "dE_rows", "stream"]
ENTRY = {"bsarec_ce_head_range_stats": STATS, "bsarec_ce_head_range_merge": MERGE, "bsarec_ce_head_range_bwd": BWD}
RANGE = [dict(col_base=-1), dict(col_base=301), dict(Vs=101, col_base=250), dict(item_size=349), dict(item_size=2 ** 31),
         dict(Vs=-1), dict(Bg=0), dict(Bg=65537), dict(d=66), dict(d=2), dict(ldh=60), dict(ldh=66), dict(h=None),
         dict(item_rows=None), dict(answers=None), dict(workspace=None), dict(h="p+4"), dict(item_rows="p+4"),
         dict(workspace="p+4"), dict(workspace_bytes=0), dict(workspace_bytes="short"),
         dict(Vs=0, col_base=350, workspace_bytes="short0"), dict(Vs=0, col_base=351)]
CASES = ([(n, c) for n in ("bsarec_ce_head_range_stats", "bsarec_ce_head_range_bwd") for c in RANGE] +
         [("bsarec_ce_head_range_stats", dict(stats=None))] +
         [("bsarec_ce_head_range_bwd", c) for c in (dict(gout=None), dict(dh_part=None), dict(dE_rows=None), dict(dh_part="p+4"),
                                                    dict(dE_rows="p+4"), dict(Vs=0, col_base=350, dh_part=None))] +
         [("bsarec_ce_head_range_merge", c) for c in (dict(world=0), dict(world=9), dict(world=-1), dict(Bg=0), dict(Bg=65537),
                                                      dict(stats_all=None), dict(workspace=None), dict(workspace="p+4"),
                                                      dict(workspace_bytes="merge_short"), dict(workspace_bytes=0),
                                                      dict(loss_rows=None), dict(loss=None))])


@pytest.mark.parametrize("name,change", CASES, ids=[f"{n[21:]}-{'-'.join(f'{k}={v}' for k, v in c.items())}" for n, c in CASES])
def test_invalid_arguments_return_negative_without_a_gpu(name, change):
    """The valid call: rows [250, 350) of 350 items for 8 sequences, d = 64, world = 2.  Every case changes it into one the
    entry point refuses on the host."""
    from bsarec_amd import _lib
    lib = _lib.load()
    buf = (C.c_byte * 4096)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16           # a 16-byte aligned host address (never dereferenced)
    need = lib.bsarec_ce_head_range_workspace_bytes(8, 100, 64)
    assert need > 8 * 8
    kw = dict(h=p, ldh=3200, item_rows=p, Bg=8, Vs=100, col_base=250, item_size=350, d=64, answers=p, stats=p, gout=p,
              workspace=p, workspace_bytes=need, dh_part=p, dE_rows=p, stats_all=p, world=2, loss_rows=p, loss=p, stream=None)
    short = {"p+4": p + 4, "short": need - 1, "short0": lib.bsarec_ce_head_range_workspace_bytes(8, 0, 64) - 1,
             "merge_short": 2 * 8 * 4 - 1}
    for k, v in change.items():
        kw[k] = short[v] if isinstance(v, str) else v
    assert getattr(lib, name)(*[kw[k] for k in ENTRY[name]]) < 0


def _ns(**kw):
    a = argparse.Namespace(item_size=301, hidden_size=64, max_seq_length=50, batch_size=32, hidden_dropout_prob=0.0,
                           attention_probs_dropout_prob=0.0, num_hidden_layers=2, num_attention_heads=2,
                           hidden_act="gelu", initializer_range=0.02, c=3, alpha=0.9, seed=42)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("kw", [dict(shard_ce_head="triton"), dict(shard_ce_head="Fused"), dict(shard_ce_head=None),
                                dict(shard_ce_head="fused", train_negatives=64),
                                dict(shard_ce_head="fused", train_negatives=64, train_lazy_adam=True)])
def test_shard_ce_head_flag_is_refused_on_the_host(kw):
    from bsarec_amd.catalogue import ShardedCatalogue
    with pytest.raises(ValueError, match="shard_ce_head"):
        ShardedCatalogue(_ns(**kw), 32, None, "cpu")          # no group, a CPU device: the flag's refusal comes first


def test_shard_ce_head_values_pass_the_flag_checks():
    """"dense", "fused" and "dense" beside the sampled head pass: what stops them on the host is the device."""
    from bsarec_amd.catalogue import SHARD_CE_HEADS, ShardedCatalogue
    assert SHARD_CE_HEADS == ("dense", "fused")
    for kw in (dict(shard_ce_head="dense"), dict(shard_ce_head="fused"), dict(shard_ce_head="dense", train_negatives=64),
               dict(shard_ce_head="fused", eval_full_rank="fused")):
        with pytest.raises(ValueError, match="runs on the GPU only"):
            ShardedCatalogue(_ns(**kw), 32, None, "cpu")
