"""The fused GRU4Rec step on the host, no GPU: the fp64 restatement (gru4rec_step_ref) against torch autograd and torch.optim.Adam
in double on the twin model, the new symbols and their bindings, the header as plain C, every argument limit of the two entry
points (they return < 0 before any HIP call), the command-line flag and the model's mode switch."""
import argparse
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import abi_cases as A
import gru4rec_step_ref as S

V, D, H, N, L, B = 23, 8, 32, 2, 5, 6


class Twin(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.item_embeddings = torch.nn.Embedding(V, D)
        self.gru_layers = torch.nn.GRU(D, H, N, bias=False, batch_first=True)
        self.dense = torch.nn.Linear(H, D)

    def calculate_loss(self, ids, pos, neg, mult):
        E = self.item_embeddings
        s = self.dense(self.gru_layers(E(ids) * mult)[0])[:, -1]
        return -torch.log(torch.sigmoid((s * E(pos)).sum(-1) - (s * E(neg)).sum(-1)) + 1e-10).mean()


def _batch():
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(1, V, (B, L), generator=g)
    ids[:2, :2] = 0
    pos = torch.randint(1, V, (B,), generator=g)
    neg = torch.randint(1, V, (B,), generator=g)
    pos[0], neg[1] = ids[0, -1], ids[1, -1]               # rows that the lookup and the head both touch
    neg[2] = pos[2]                                       # a row whose head terms cancel
    neg[3] = pos[4]                                       # a negative that is another row's answer
    return ids, pos, neg


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_reference_equals_autograd_and_torch_adam_in_double(wd):
    torch.manual_seed(9)
    twin = Twin().double()
    with torch.no_grad():
        twin.item_embeddings.weight.mul_(0.5)
        twin.dense.bias.normal_(0.0, 0.1)
    assert [k for k, _ in twin.named_parameters()] == S.keys(N)
    params = {k: p.detach().numpy().copy() for k, p in twin.named_parameters()}
    ids, pos, neg = _batch()
    opt = torch.optim.Adam(twin.parameters(), lr=1e-2, weight_decay=wd)
    st = S.adam_state(lr=1e-2, weight_decay=wd)
    for step in range(1, 4):
        mult = S.dropout_mult(B, L, D, 0.5, 1234567, step)
        assert set(np.unique(mult)) == {0.0, 2.0}
        rloss, rgrads = S.loss_and_grads(params, ids.numpy(), pos.numpy(), neg.numpy(), H, N, mult)
        opt.zero_grad()
        loss = twin.calculate_loss(ids, pos, neg, torch.from_numpy(mult))
        loss.backward()
        assert abs(rloss - loss.item()) <= 1e-12
        for k, p in twin.named_parameters():
            assert np.abs(rgrads[k] - p.grad.numpy()).max() <= 1e-12, (step, k)
        opt.step()
        assert S.train_step(params, st, ids.numpy(), pos.numpy(), neg.numpy(), H, N, mult) == rloss
        for k, p in twin.named_parameters():
            assert np.abs(params[k] - p.detach().numpy()).max() <= 1e-12, (step, k)
    assert st.t == 3


NAMES = ("bsarec_gru4rec_workspace_bytes", "bsarec_gru4rec_loss_grad", "bsarec_gru4rec_train_step")


def test_symbols_are_exported_and_bound():
    from bsarec_amd import _lib
    A.check_symbols(NAMES, {"bsarec_gru4rec_loss_grad": 14, "bsarec_gru4rec_train_step": 11}, _lib.Gru4RecConfig,
                    ["gru", "item_size", "dropout"], C.sizeof(_lib.GruConfig) + 8)


def test_header_block_is_plain_c99_and_links(tmp_path):
    src = r"""
#include "bsarec_hip.h"
#include <stdio.h>
int main(void) {
    bsarec_gru4rec_config_t cfg = {{256, 50, 64, 64, 2, 64}, 3417, 0.5f};
    long ws = bsarec_gru4rec_workspace_bytes(&cfg), gws = bsarec_gru_workspace_bytes(&cfg.gru, 1);
    int (*lg)(const bsarec_gru4rec_config_t *, const float *, const float *, const int64_t *, const int64_t *, const int64_t *,
              void *, int, float *, float *, float *, void *, long, void *) = bsarec_gru4rec_loss_grad;
    int (*ts)(const bsarec_gru4rec_config_t *, const int64_t *, const int64_t *, const int64_t *, const bsarec_adam_t *,
              const bsarec_adam_t *, void *, float *, void *, long, void *) = bsarec_gru4rec_train_step;
    long bad;
    cfg.item_size = 1;
    bad = bsarec_gru4rec_workspace_bytes(&cfg);
    printf("%d %ld %ld %ld\n", bsarec_abi_version(), ws, gws, bad);
    return (lg && ts && bsarec_abi_version() == 10 && ws > gws && gws > 0 && bad < 0) ? 0 : 1;
}
"""
    ver, ws, gws, bad = A.run_c99(tmp_path, src)
    T, Bq, d, Vq = 256 * 50, 256, 64, 3417
    assert ver == 10 and ws == gws + 4 * (2 * T * d + 2 * Bq * d + 2 * Bq + 2 * Vq * d)


GOOD = dict(batch=8, seq_len=10, input_size=64, hidden_size=64, num_layers=2, out_size=64, item_size=50, dropout=0.5)
BAD_CFG = [dict(batch=0), dict(batch=65537), dict(seq_len=0), dict(seq_len=257), dict(input_size=66, out_size=66),
           dict(input_size=260, out_size=260), dict(hidden_size=48), dict(num_layers=0), dict(num_layers=5),
           dict(out_size=32), dict(out_size=0), dict(input_size=32), dict(item_size=1), dict(item_size=0), dict(item_size=-7),
           dict(dropout=-0.1), dict(dropout=1.0), dict(dropout=1.5), dict(dropout=float("nan"))]
LOSS_GRAD = ["cfg", "item_emb", "weights", "ids", "answers", "neg_answers", "state", "train", "loss_out", "d_item_emb", "dweights",
             "workspace", "workspace_bytes", "stream"]
TRAIN_STEP = ["cfg", "ids", "answers", "neg_answers", "adam_items", "adam_weights", "state", "loss_out", "workspace",
              "workspace_bytes", "stream"]
ENTRY = {"bsarec_gru4rec_loss_grad": LOSS_GRAD, "bsarec_gru4rec_train_step": TRAIN_STEP}
PTRS16 = {"bsarec_gru4rec_loss_grad": ["item_emb", "weights", "d_item_emb", "dweights", "workspace"],
          "bsarec_gru4rec_train_step": ["workspace"]}
PTRS8 = ["ids", "answers", "neg_answers", "state"]
CASES = A.step_cases(ENTRY, BAD_CFG, PTRS16, PTRS8)


def _cfg(**kw):
    from bsarec_amd import _lib
    c = dict(GOOD)
    c.update(kw)
    gru = _lib.GruConfig(*[c[k] for k in ("batch", "seq_len", "input_size", "hidden_size", "num_layers", "out_size")])
    return _lib.Gru4RecConfig(gru, c["item_size"], c["dropout"])


SPEC = A.spec(GOOD, _cfg, ENTRY, PTRS16, PTRS8, need=lambda lib: lib.bsarec_gru4rec_workspace_bytes(_cfg()),
              adam_n=lambda lib: {"adam_items": GOOD["item_size"] * GOOD["input_size"],
                                  "adam_weights": lib.bsarec_gru_weight_floats(_cfg().gru)})


def test_workspace_query():
    from bsarec_amd import _lib
    lib = _lib.load()
    assert lib.bsarec_gru4rec_workspace_bytes(_cfg()) > lib.bsarec_gru_workspace_bytes(_cfg().gru, 1) > 0
    assert lib.bsarec_gru4rec_workspace_bytes(_cfg(dropout=0.0)) == lib.bsarec_gru4rec_workspace_bytes(_cfg())
    assert lib.bsarec_gru4rec_workspace_bytes(_cfg(item_size=2)) > 0
    assert lib.bsarec_gru4rec_workspace_bytes(None) < 0
    for change in BAD_CFG:
        assert lib.bsarec_gru4rec_workspace_bytes(_cfg(**change)) < 0, change


@pytest.mark.parametrize("name,change", CASES, ids=A.ids(CASES, "bsarec_gru4rec_"))
def test_invalid_arguments_return_negative_without_a_gpu(name, change):
    assert A.call(SPEC, name, change) < 0


def _args(**kw):
    a = argparse.Namespace(item_size=301, hidden_size=64, gru_hidden_size=64, num_hidden_layers=2, max_seq_length=20,
                           hidden_dropout_prob=0.5, initializer_range=0.02)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_command_line_flag():
    A.check_flag("gru_step", "GRU4Rec")


def test_mode_switch_on_the_host():
    from bsarec_amd import GRU4RecModel
    assert GRU4RecModel.torch_optim is True
    default, torch_mode, fused = GRU4RecModel(_args()), GRU4RecModel(_args(gru_step="torch")), GRU4RecModel(_args(gru_step="fused"))
    assert default.gru_step == torch_mode.gru_step == "torch" and default.torch_optim is True and torch_mode.torch_optim is True
    assert fused.gru_step == "fused" and fused.torch_optim is False and fused.needs_negatives is True
    assert list(fused.state_dict()) == list(default.state_dict())
    with pytest.raises(ValueError, match="gru_step"):
        GRU4RecModel(_args(gru_step="bogus"))
    ids = torch.randint(1, 301, (3, 20))
    with pytest.raises(RuntimeError, match="torch.optim.Adam"):
        default.train_step(ids, ids[:, 0], ids[:, 1])
    with pytest.raises(RuntimeError, match="MI355X"):               # no CPU path for the fused step either
        fused.train_step(ids, ids[:, 0], ids[:, 1])
    with pytest.raises(RuntimeError, match="MI355X"):
        fused.loss_and_grads(ids, ids[:, 0], ids[:, 1])
