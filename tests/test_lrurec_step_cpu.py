"""The fused LRURec step on the host, no GPU: the fp64 restatement (lrurec_step_ref) against torch autograd and torch.optim.Adam in
double on a twin whose recurrent layer runs on torch complex tensors, the new symbols and their bindings, the header as plain C,
the weight count against ``lrurec_param_shapes``, every argument limit of the two entry points (they return < 0 before any HIP
call), the command-line flag and the model's mode switch with its flat weight array."""
import argparse
import ctypes as C
import math
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import abi_cases as A
import block_step_twin as W
import lru_ref as R
import lrurec_step_ref as S

SHAPES = [(11, 4, 1, 1, 3), (23, 12, 2, 7, 5), (17, 8, 1, 20, 4)]          # V, d, N, L, B


# the layer as block_step_twin takes it
LRU = types.SimpleNamespace(prefix="lru", names=R.weight_shapes, layer=R.torch_complex_layer,
                            weights=lambda rng, d: R.split_weights(R.random_weights(rng, d).astype(np.float64), d),
                            keys=S.keys, ragged_ids=R.ragged_ids, loss_and_grads=S.loss_and_grads, train_step=S.train_step)


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "V%d-d%d-N%d-L%d-B%d" % s)
def test_reference_equals_autograd_and_torch_adam_in_double(shape, wd):
    W.reference_equals_the_twin(LRU, shape, wd)


def test_philox_multipliers():
    m = S.dropout_mults(3, 5, 8, 2, 0.5, 1234567, 2)
    assert len(m) == 5 and all(set(np.unique(a)) == {0.0, 2.0} and a.shape == (3, 5, 8) for a in m)
    assert not np.array_equal(m[0], m[1])
    assert all(np.array_equal(a, np.ones((3, 5, 8))) for a in S.dropout_mults(3, 5, 8, 2, 0.0, 1, 1))


NAMES = ("bsarec_lrurec_weight_floats", "bsarec_lrurec_workspace_bytes", "bsarec_lrurec_loss_grad", "bsarec_lrurec_train_step")


def test_symbols_are_exported_and_bound():
    from bsarec_amd import _lib
    A.check_symbols(NAMES, {"bsarec_lrurec_loss_grad": 13, "bsarec_lrurec_train_step": 10}, _lib.LruRecConfig,
                    ["lru", "layers", "item_size", "dropout", "ln_eps"], C.sizeof(_lib.LruConfig) + 16)


def test_header_block_is_plain_c99_and_links(tmp_path):
    src = r"""
#include "bsarec_hip.h"
#include <stdio.h>
int main(void) {
    bsarec_lrurec_config_t cfg = {{256, 50, 64}, 2, 3417, 0.5f, 1e-12f};
    long ws = bsarec_lrurec_workspace_bytes(&cfg), lws = bsarec_lru_workspace_bytes(&cfg.lru, 1);
    long nw = bsarec_lrurec_weight_floats(&cfg);
    int (*lg)(const bsarec_lrurec_config_t *, const float *, const float *, const int64_t *, const int64_t *, void *, int,
              float *, float *, float *, void *, long, void *) = bsarec_lrurec_loss_grad;
    int (*ts)(const bsarec_lrurec_config_t *, const int64_t *, const int64_t *, const bsarec_adam_t *, const bsarec_adam_t *,
              void *, float *, void *, long, void *) = bsarec_lrurec_train_step;
    long bad;
    cfg.layers = 0;
    bad = bsarec_lrurec_workspace_bytes(&cfg);
    printf("%d %ld %ld %ld %ld\n", bsarec_abi_version(), ws, lws, nw, bad);
    return (lg && ts && bsarec_abi_version() == 10 && ws > 2 * lws && lws > 0 && bad < 0) ? 0 : 1;
}
"""
    ver, ws, lws, nw, bad = A.run_c99(tmp_path, src)
    assert ver == 10 and nw == 2 * 64 + 2 * (12 * 64 * 64 + 15 * 64)


@pytest.mark.parametrize("d,N", [(4, 1), (64, 2), (100, 3), (256, 16)])
def test_weight_floats_are_the_sum_of_the_param_shapes(d, N):
    from bsarec_amd import _lib
    from bsarec_amd.lrurec import lru_param_shapes, lrurec_param_shapes
    shapes = lrurec_param_shapes(d, N)
    total = sum(math.prod(s) for s in shapes.values())
    cfg = _lib.LruRecConfig(_lib.LruConfig(8, 10, d), N, 50, 0.5, 1e-12)
    assert _lib.load().bsarec_lrurec_weight_floats(cfg) == total == 2 * d + N * (12 * d * d + 15 * d)
    assert list(shapes) == S.keys(N, d)[1:] and len(shapes) == 2 + 15 * N
    off = 0
    for k, s in shapes.items():                                  # every tensor at a multiple of 4 floats
        assert off % 4 == 0, k
        off += math.prod(s)
    lru = list(lru_param_shapes(d).items())
    assert [(k.split(".lru.")[1], s) for k, s in shapes.items() if ".blocks.0.lru." in k and "LayerNorm" not in k] == lru


GOOD = dict(batch=8, seq_len=10, width=64, layers=2, item_size=50, dropout=0.5, ln_eps=1e-12)
BAD_CFG = [dict(batch=0), dict(batch=65537), dict(seq_len=0), dict(seq_len=257), dict(width=0), dict(width=66), dict(width=260),
           dict(layers=0), dict(layers=-1), dict(layers=17), dict(item_size=1), dict(item_size=0), dict(item_size=-7),
           dict(dropout=-0.1), dict(dropout=1.0), dict(dropout=1.5), dict(dropout=float("nan")),
           dict(ln_eps=0.0), dict(ln_eps=-1e-12), dict(ln_eps=float("nan"))]
LOSS_GRAD = ["cfg", "item_emb", "weights", "ids", "answers", "state", "train", "loss_out", "d_item_emb", "dweights", "workspace",
             "workspace_bytes", "stream"]
TRAIN_STEP = ["cfg", "ids", "answers", "adam_items", "adam_weights", "state", "loss_out", "workspace", "workspace_bytes", "stream"]
ENTRY = {"bsarec_lrurec_loss_grad": LOSS_GRAD, "bsarec_lrurec_train_step": TRAIN_STEP}
PTRS16 = {"bsarec_lrurec_loss_grad": ["item_emb", "weights", "d_item_emb", "dweights", "workspace"],
          "bsarec_lrurec_train_step": ["workspace"]}
PTRS8 = ["ids", "answers", "state"]
CASES = A.step_cases(ENTRY, BAD_CFG, PTRS16, PTRS8)


def _cfg(**kw):
    from bsarec_amd import _lib
    c = dict(GOOD)
    c.update(kw)
    return _lib.LruRecConfig(_lib.LruConfig(c["batch"], c["seq_len"], c["width"]), c["layers"], c["item_size"], c["dropout"],
                             c["ln_eps"])


SPEC = A.spec(GOOD, _cfg, ENTRY, PTRS16, PTRS8, need=lambda lib: lib.bsarec_lrurec_workspace_bytes(_cfg()),
              adam_n=lambda lib: {"adam_items": GOOD["item_size"] * GOOD["width"],
                                  "adam_weights": lib.bsarec_lrurec_weight_floats(_cfg())})


def test_workspace_query():
    from bsarec_amd import _lib
    lib = _lib.load()
    one, two = lib.bsarec_lrurec_workspace_bytes(_cfg(layers=1)), lib.bsarec_lrurec_workspace_bytes(_cfg())
    assert two > one > lib.bsarec_lru_workspace_bytes(_cfg().lru, 1) > 0 and two % 16 == 0
    assert lib.bsarec_lrurec_workspace_bytes(_cfg(dropout=0.0)) == two
    assert lib.bsarec_lrurec_workspace_bytes(_cfg(item_size=2)) > 0 and lib.bsarec_lrurec_workspace_bytes(_cfg(layers=16)) > 0
    assert lib.bsarec_lrurec_workspace_bytes(None) < 0 and lib.bsarec_lrurec_weight_floats(None) < 0
    for change in BAD_CFG:
        assert lib.bsarec_lrurec_workspace_bytes(_cfg(**change)) < 0, change
        assert lib.bsarec_lrurec_weight_floats(_cfg(**change)) < 0, change


@pytest.mark.parametrize("name,change", CASES, ids=A.ids(CASES, "bsarec_lrurec_"))
def test_invalid_arguments_return_negative_without_a_gpu(name, change):
    assert A.call(SPEC, name, change) < 0


def _args(**kw):
    a = argparse.Namespace(item_size=41, hidden_size=8, num_hidden_layers=2, max_seq_length=6, hidden_dropout_prob=0.5,
                           initializer_range=0.02)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_command_line_flag():
    A.check_flag("lru_step", "LRURec")


def test_mode_switch_and_the_flat_array_on_the_host():
    from bsarec_amd import LRURecModel
    from bsarec_amd.lrurec import lrurec_param_shapes
    W.mode_switch_and_the_flat_array(LRURecModel, _args, "lru_step", lrurec_param_shapes(8, 2), S.keys(2, 8), "lru", "nu_log",
                                     4 * 8 * 8 + 6 * 8)
