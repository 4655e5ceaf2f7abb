"""The fused Mamba4Rec step on the host, no GPU: the fp64 restatement (mamba4rec_step_ref) against torch autograd and
torch.optim.Adam in double on a twin whose state-space layer is mamba_ref.torch_layer, the new symbols and their bindings, the
header as plain C, the weight count against ``mamba4rec_param_shapes``, every argument limit of the two entry points (they return
< 0 before any HIP call), the command-line flag and the model's mode switch with its flat weight array."""
import argparse
import ctypes as C
import math
import types

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import abi_cases as A
import block_step_twin as W
import mamba_ref as M
import mamba4rec_step_ref as S

# V, d, N, L, B; expand, d_state, d_conv, dt_rank
SHAPES = [((11, 4, 1, 1, 3), (1, 4, 2, 4)), ((23, 12, 2, 7, 5), (2, 8, 4, 4)), ((17, 8, 1, 20, 4), (2, 16, 3, 4))]


def _twin(hyper):
    """The layer at ``hyper`` as block_step_twin takes it."""
    return types.SimpleNamespace(
        prefix="mamba", names=lambda d: M.weight_shapes(d, *hyper), layer=lambda x, ids, w: M.torch_layer(x, ids, w, hyper),
        weights=lambda rng, d: M.split_weights(M.random_weights(rng, d, *hyper, std=0.3).astype(np.float64), d, *hyper),
        keys=lambda N, d: S.keys(N, hyper, d), ragged_ids=M.ragged_ids,
        loss_and_grads=lambda params, ids, ans, N, mults: S.loss_and_grads(params, ids, ans, N, hyper, mults),
        train_step=lambda params, st, ids, ans, N, mults: S.train_step(params, st, ids, ans, N, hyper, mults))


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("shape,hyper", SHAPES, ids=lambda s: "-".join(str(v) for v in s))
def test_reference_equals_autograd_and_torch_adam_in_double(shape, hyper, wd):
    W.reference_equals_the_twin(_twin(hyper), shape, wd)


NAMES = ("bsarec_mamba4rec_weight_floats", "bsarec_mamba4rec_workspace_bytes", "bsarec_mamba4rec_loss_grad",
         "bsarec_mamba4rec_train_step")


def test_symbols_are_exported_and_bound():
    from bsarec_amd import _lib
    A.check_symbols(NAMES, {"bsarec_mamba4rec_loss_grad": 13, "bsarec_mamba4rec_train_step": 10}, _lib.Mamba4RecConfig,
                    ["mamba", "layers", "item_size", "dropout", "ln_eps"], C.sizeof(_lib.MambaConfig) + 16)
    assert _lib.EXPORTS["bsarec_mamba4rec_loss_grad"][1][1:] == _lib.EXPORTS["bsarec_lrurec_loss_grad"][1][1:]
    assert _lib.EXPORTS["bsarec_mamba4rec_train_step"][1][1:] == _lib.EXPORTS["bsarec_lrurec_train_step"][1][1:]


def test_header_block_is_plain_c99_and_links(tmp_path):
    src = r"""
#include "bsarec_hip.h"
#include <stdio.h>
int main(void) {
    bsarec_mamba4rec_config_t cfg = {{256, 50, 64, 2, 16, 4, 4}, 2, 3417, 0.5f, 1e-12f};
    long ws = bsarec_mamba4rec_workspace_bytes(&cfg), lws = bsarec_mamba_workspace_bytes(&cfg.mamba, 1);
    long nw = bsarec_mamba4rec_weight_floats(&cfg), m = bsarec_mamba_weight_floats(&cfg.mamba);
    int (*lg)(const bsarec_mamba4rec_config_t *, const float *, const float *, const int64_t *, const int64_t *, void *, int,
              float *, float *, float *, void *, long, void *) = bsarec_mamba4rec_loss_grad;
    int (*ts)(const bsarec_mamba4rec_config_t *, const int64_t *, const int64_t *, const bsarec_adam_t *, const bsarec_adam_t *,
              void *, float *, void *, long, void *) = bsarec_mamba4rec_train_step;
    long bad;
    cfg.layers = 0;
    bad = bsarec_mamba4rec_workspace_bytes(&cfg);
    printf("%d %ld %ld %ld %ld %ld\n", bsarec_abi_version(), ws, lws, nw, m, bad);
    return (lg && ts && bsarec_abi_version() == 10 && ws > 2 * lws && lws > 0 && bad < 0) ? 0 : 1;
}
"""
    ver, ws, lws, nw, m, bad = A.run_c99(tmp_path, src)
    assert ver == 10 and m == M.weight_floats(64, 2, 16, 4, 4) and nw == 2 * 64 + 2 * (m + 8 * 64 * 64 + 9 * 64)


@pytest.mark.parametrize("d,N,hyper", [(4, 1, (1, 4, 2, 4)), (64, 2, (2, 16, 4, 4)), (100, 3, (2, 16, 3, 8)),
                                       (256, 16, (2, 32, 4, 16)), (12, 2, (1, 8, 3, 64))])
def test_weight_floats_are_the_sum_of_the_param_shapes(d, N, hyper):
    from bsarec_amd import _lib
    from bsarec_amd.mamba4rec import mamba4rec_param_shapes, mamba_param_shapes
    shapes = mamba4rec_param_shapes(d, N, *hyper)
    total = sum(math.prod(s) for s in shapes.values())
    cfg = _lib.Mamba4RecConfig(_lib.MambaConfig(8, 10, d, *hyper), N, 50, 0.5, 1e-12)
    Mw = _lib.load().bsarec_mamba_weight_floats(cfg.mamba)
    assert Mw == M.weight_floats(d, *hyper)
    assert _lib.load().bsarec_mamba4rec_weight_floats(cfg) == total == 2 * d + N * (Mw + 8 * d * d + 9 * d)
    assert list(shapes) == S.flat_keys(N, hyper, d) and sorted(shapes) == sorted(S.keys(N, hyper, d)[1:])
    assert len(shapes) == 2 + 17 * N
    off = 0
    for k, s in shapes.items():                                  # every tensor at a multiple of 4 floats
        assert off % 4 == 0, k
        off += math.prod(s)
    layer = list(mamba_param_shapes(d, *hyper).items())
    assert [(k.split(".mamba.")[1], s) for k, s in shapes.items() if ".blocks.0.mamba." in k and "LayerNorm" not in k] == layer


GOOD = dict(batch=8, seq_len=10, width=64, expand=2, d_state=16, d_conv=4, dt_rank=4, layers=2, item_size=50, dropout=0.5,
            ln_eps=1e-12)
BAD_CFG = [dict(batch=0), dict(batch=65537), dict(seq_len=0), dict(seq_len=257), dict(width=0), dict(width=66), dict(width=260),
           dict(expand=0), dict(expand=3), dict(d_state=5), dict(d_state=64), dict(d_conv=1), dict(d_conv=5),
           dict(dt_rank=0), dict(dt_rank=6), dict(dt_rank=68),
           dict(layers=0), dict(layers=-1), dict(layers=17), dict(item_size=1), dict(item_size=0), dict(item_size=-7),
           dict(dropout=-0.1), dict(dropout=1.0), dict(dropout=1.5), dict(dropout=float("nan")),
           dict(ln_eps=0.0), dict(ln_eps=-1e-12), dict(ln_eps=float("nan"))]
LOSS_GRAD = ["cfg", "item_emb", "weights", "ids", "answers", "state", "train", "loss_out", "d_item_emb", "dweights", "workspace",
             "workspace_bytes", "stream"]
TRAIN_STEP = ["cfg", "ids", "answers", "adam_items", "adam_weights", "state", "loss_out", "workspace", "workspace_bytes", "stream"]
ENTRY = {"bsarec_mamba4rec_loss_grad": LOSS_GRAD, "bsarec_mamba4rec_train_step": TRAIN_STEP}
PTRS16 = {"bsarec_mamba4rec_loss_grad": ["item_emb", "weights", "d_item_emb", "dweights", "workspace"],
          "bsarec_mamba4rec_train_step": ["workspace"]}
PTRS8 = ["ids", "answers", "state"]
CASES = A.step_cases(ENTRY, BAD_CFG, PTRS16, PTRS8)


def _cfg(**kw):
    from bsarec_amd import _lib
    c = dict(GOOD)
    c.update(kw)
    return _lib.Mamba4RecConfig(_lib.MambaConfig(c["batch"], c["seq_len"], c["width"], c["expand"], c["d_state"], c["d_conv"],
                                                 c["dt_rank"]), c["layers"], c["item_size"], c["dropout"], c["ln_eps"])


SPEC = A.spec(GOOD, _cfg, ENTRY, PTRS16, PTRS8, need=lambda lib: lib.bsarec_mamba4rec_workspace_bytes(_cfg()),
              adam_n=lambda lib: {"adam_items": GOOD["item_size"] * GOOD["width"],
                                  "adam_weights": lib.bsarec_mamba4rec_weight_floats(_cfg())})


def test_workspace_query():
    from bsarec_amd import _lib
    lib = _lib.load()
    sizes = [lib.bsarec_mamba4rec_workspace_bytes(_cfg(layers=n)) for n in (1, 2, 3, 16)]
    layer = lib.bsarec_mamba_workspace_bytes(_cfg().mamba, 1)
    assert layer > 0 and all(b > a for a, b in zip(sizes, sizes[1:]))                  # monotone in N
    assert all(s > n * layer and s % 16 == 0 for s, n in zip(sizes, (1, 2, 3, 16)))     # larger than N Mamba workspaces
    two = sizes[1]
    assert lib.bsarec_mamba4rec_workspace_bytes(_cfg(dropout=0.0)) == two
    assert lib.bsarec_mamba4rec_workspace_bytes(_cfg(item_size=2)) > 0
    assert lib.bsarec_mamba4rec_workspace_bytes(None) < 0 and lib.bsarec_mamba4rec_weight_floats(None) < 0
    for change in BAD_CFG:
        assert lib.bsarec_mamba4rec_workspace_bytes(_cfg(**change)) < 0, change
        assert lib.bsarec_mamba4rec_weight_floats(_cfg(**change)) < 0, change


@pytest.mark.parametrize("name,change", CASES, ids=A.ids(CASES, "bsarec_mamba4rec"))       # "_loss_grad-...": the ids as they are
def test_invalid_arguments_return_negative_without_a_gpu(name, change):
    assert A.call(SPEC, name, change) < 0


def _args(**kw):
    a = argparse.Namespace(item_size=41, hidden_size=8, num_hidden_layers=2, max_seq_length=6, hidden_dropout_prob=0.5,
                           initializer_range=0.02)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_command_line_flag():
    A.check_flag("mamba_step", "Mamba4Rec")


def test_mode_switch_and_the_flat_array_on_the_host():
    from bsarec_amd import Mamba4RecModel
    from bsarec_amd.mamba4rec import mamba4rec_param_shapes
    hyper = (2, 16, 4, 4)                                          # the layer's defaults at d = 8
    W.mode_switch_and_the_flat_array(Mamba4RecModel, _args, "mamba_step", mamba4rec_param_shapes(8, 2, *hyper),
                                     S.keys(2, hyper, 8), "mamba", "in_proj.weight", M.weight_floats(8, *hyper))
