"""The fused Caser step on the host, no GPU: the fp64 restatement (caser_step_ref) against torch autograd and torch.optim.Adam in
double on the twin model, the new symbols and their bindings, the header as plain C, every argument limit of the entry points (they
return < 0 before any HIP call), the command-line flag and the model's mode switch."""
import argparse
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import abi_cases as A  # noqa: E402
import caser_step_ref as S  # noqa: E402
from test_caser_cpu import Twin  # noqa: E402

V, D, L, B, NH, NV = 23, 8, 5, 6, 4, 2
FZ = NV * D + NH * L


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


def _twin_loss(twin, ids, pos, neg, mult):
    E = twin.item_embeddings
    s = torch.relu(twin.fc1(twin.conv(E(ids)) * mult))
    return -torch.log(torch.sigmoid((s * E(pos)).sum(-1) - (s * E(neg)).sum(-1)) + 1e-10).mean()


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_reference_equals_autograd_and_torch_adam_in_double(wd):
    torch.manual_seed(9)
    twin = Twin(V, L, D, NH, NV).double()
    with torch.no_grad():
        twin.item_embeddings.weight.mul_(0.8)
        twin.fc1.bias.normal_(0.0, 0.1)
    assert [k for k, _ in twin.named_parameters()] == S.keys(L)
    params = {k: p.detach().numpy().copy() for k, p in twin.named_parameters()}
    assert S.shape_of(params) == (L, D, NH, NV)
    ids, pos, neg = _batch()
    opt = torch.optim.Adam(twin.parameters(), lr=1e-2, weight_decay=wd)
    st = S.adam_state(lr=1e-2, weight_decay=wd)
    for step in range(1, 4):
        mult = S.dropout_mult(B, FZ, 0.5, 1234567, step)              # an explicit mask: the library's stream at this step
        assert set(np.unique(mult)) == {0.0, 2.0}
        rloss, s, rgrads = S.loss_and_grads(params, ids.numpy(), pos.numpy(), neg.numpy(), mult)
        assert (s > 0).any() and (s == 0).any()                       # the ReLU takes both branches
        opt.zero_grad()
        loss = _twin_loss(twin, ids, pos, neg, torch.from_numpy(mult))
        loss.backward()
        assert abs(rloss - loss.item()) <= 1e-12
        for k, p in twin.named_parameters():
            assert rgrads[k].shape == tuple(p.shape)
            assert np.abs(rgrads[k] - p.grad.numpy()).max() <= 1e-12, (step, k)
        opt.step()
        assert S.train_step(params, st, ids.numpy(), pos.numpy(), neg.numpy(), mult) == rloss
        for k, p in twin.named_parameters():
            assert np.abs(params[k] - p.detach().numpy()).max() <= 1e-12, (step, k)
    assert st.t == 3


def test_dropout_mult_is_the_oracle_stream_of_site_0():
    from oracle import bsarec_oracle as O
    m = S.dropout_mult(3, 8, 0.5, 77, 2)
    assert np.array_equal(m.reshape(-1) > 0, O.dropout_keep(24, 0.5, 77, 2, 0))
    assert np.array_equal(S.dropout_mult(3, 8, 0.0, 77, 2), np.ones((3, 8)))


NAMES = ("bsarec_caser_fc_floats", "bsarec_caser_fc_workspace_bytes", "bsarec_caser_fc_fwd", "bsarec_caser_fc_bwd",
         "bsarec_caser_step_workspace_bytes", "bsarec_caser_loss_grad", "bsarec_caser_train_step")


def test_symbols_are_exported_and_bound():
    from bsarec_amd import _lib
    nargs = {"bsarec_caser_fc_fwd": 12, "bsarec_caser_fc_bwd": 15, "bsarec_caser_loss_grad": 16, "bsarec_caser_train_step": 12}
    A.check_symbols(NAMES, nargs, _lib.CaserStepConfig, ["conv", "item_size", "dropout"],      # the eighth new name: the struct
                    C.sizeof(_lib.CaserConfig) + 8)


def test_header_block_is_plain_c99_and_links(tmp_path):
    src = r"""
#include "bsarec_hip.h"
#include <stdio.h>
int main(void) {
    bsarec_caser_step_config_t cfg = {{256, 50, 64, 16, 4}, 3417, 0.5f};
    long ws = bsarec_caser_step_workspace_bytes(&cfg), cws = bsarec_caser_workspace_bytes(&cfg.conv, 1);
    long fc = bsarec_caser_fc_floats(&cfg.conv), fws = bsarec_caser_fc_workspace_bytes(256, 1056, 64);
    int (*ff)(int, int, int, const float *, const float *, const void *, int, float, float *, void *, long, void *) =
        bsarec_caser_fc_fwd;
    int (*fb)(int, int, int, const float *, const float *, const float *, const float *, const void *, int, float, float *,
              float *, void *, long, void *) = bsarec_caser_fc_bwd;
    int (*lg)(const bsarec_caser_step_config_t *, const float *, const float *, const float *, const int64_t *, const int64_t *,
              const int64_t *, void *, int, float *, float *, float *, float *, void *, long, void *) = bsarec_caser_loss_grad;
    int (*ts)(const bsarec_caser_step_config_t *, const int64_t *, const int64_t *, const int64_t *, const bsarec_adam_t *,
              const bsarec_adam_t *, const bsarec_adam_t *, void *, float *, void *, long, void *) = bsarec_caser_train_step;
    long bad;
    cfg.item_size = 1;
    bad = bsarec_caser_step_workspace_bytes(&cfg);
    printf("%d %ld %ld %ld %ld %ld\n", bsarec_abi_version(), ws, cws, fc, fws, bad);
    return (ff && fb && lg && ts && bsarec_abi_version() == 10 && ws > cws && cws > 0 && bad < 0) ? 0 : 1;
}
"""
    ver, ws, cws, fc, fws, bad = A.run_c99(tmp_path, src)
    Bq, Lq, d, Vq, Fq = 256, 50, 64, 3417, 4 * 64 + 16 * 50
    T = Bq * Lq
    assert ver == 10 and fc == d * Fq + d and fws == 4 * Bq * Fq
    assert ws == cws + 4 * (2 * T * d + 3 * Bq * Fq + 2 * Bq * d + 2 * Bq + 2 * Vq * d)


GOOD = dict(batch=8, seq_len=12, width=16, n_h=8, n_v=3, item_size=50, dropout=0.5)
CONV = ("batch", "seq_len", "width", "n_h", "n_v")
BAD_CFG = [dict(batch=0), dict(batch=65537), dict(seq_len=0), dict(seq_len=257), dict(width=0), dict(width=6), dict(width=260),
           dict(n_h=0), dict(n_h=12), dict(n_h=64), dict(n_v=0), dict(n_v=17), dict(item_size=1), dict(item_size=0),
           dict(item_size=-7), dict(dropout=-0.1), dict(dropout=1.0), dict(dropout=1.5), dict(dropout=float("nan"))]
LOSS_GRAD = ["cfg", "item_emb", "weights", "fc", "ids", "answers", "neg_answers", "state", "train", "loss_out", "d_item_emb",
             "dweights", "dfc", "workspace", "workspace_bytes", "stream"]
TRAIN_STEP = ["cfg", "ids", "answers", "neg_answers", "adam_items", "adam_weights", "adam_fc", "state", "loss_out", "workspace",
              "workspace_bytes", "stream"]
ENTRY = {"bsarec_caser_loss_grad": LOSS_GRAD, "bsarec_caser_train_step": TRAIN_STEP}
PTRS16 = {"bsarec_caser_loss_grad": ["item_emb", "weights", "fc", "d_item_emb", "dweights", "dfc", "workspace"],
          "bsarec_caser_train_step": ["workspace"]}
PTRS8 = ["ids", "answers", "neg_answers", "state"]
ADAMS = ("adam_items", "adam_weights", "adam_fc")
CASES = A.step_cases(ENTRY, BAD_CFG, PTRS16, PTRS8, ADAMS,
                     hyper=[{"adam_weights.lr": 2e-3}, {"adam_fc.lr": 2e-3}, {"adam_weights.beta1": 0.8}, {"adam_fc.beta1": 0.8},
                            {"adam_items.beta2": 0.99}, {"adam_fc.beta2": 0.99}])


def _cfg(**kw):
    from bsarec_amd import _lib
    c = dict(GOOD)
    c.update(kw)
    return _lib.CaserStepConfig(_lib.CaserConfig(*[c[k] for k in CONV]), c["item_size"], c["dropout"])


SPEC = A.spec(GOOD, _cfg, ENTRY, PTRS16, PTRS8, need=lambda lib: lib.bsarec_caser_step_workspace_bytes(_cfg()),
              adam_n=lambda lib: {"adam_items": GOOD["item_size"] * GOOD["width"],
                                  "adam_weights": lib.bsarec_caser_weight_floats(_cfg().conv),
                                  "adam_fc": lib.bsarec_caser_fc_floats(_cfg().conv)})


def test_workspace_and_size_queries():
    from bsarec_amd import _lib
    lib = _lib.load()
    assert lib.bsarec_caser_step_workspace_bytes(_cfg()) > lib.bsarec_caser_workspace_bytes(_cfg().conv, 1) > 0
    assert lib.bsarec_caser_step_workspace_bytes(_cfg(dropout=0.0)) == lib.bsarec_caser_step_workspace_bytes(_cfg())
    assert lib.bsarec_caser_step_workspace_bytes(_cfg(item_size=2)) > 0
    assert lib.bsarec_caser_step_workspace_bytes(None) < 0
    for change in BAD_CFG:
        assert lib.bsarec_caser_step_workspace_bytes(_cfg(**change)) < 0, change
    F = 3 * 16 + 8 * 12
    assert lib.bsarec_caser_fc_floats(_cfg().conv) == 16 * F + 16
    assert lib.bsarec_caser_fc_floats(None) < 0 and lib.bsarec_caser_fc_floats(_cfg(width=6).conv) < 0
    assert lib.bsarec_caser_fc_workspace_bytes(8, F, 16) == 4 * 8 * F
    assert lib.bsarec_caser_fc_workspace_bytes(1, 4, 4) == 16 and lib.bsarec_caser_fc_workspace_bytes(65536, 12288, 256) > 0
    for shape in FC_BAD_SHAPES:
        assert lib.bsarec_caser_fc_workspace_bytes(*shape) < 0, shape


@pytest.mark.parametrize("name,change", CASES, ids=A.ids(CASES, "bsarec_caser_"))
def test_invalid_arguments_return_negative_without_a_gpu(name, change):
    assert A.call(SPEC, name, change) < 0


FC_FWD = ["batch", "features", "width", "z", "fc", "state", "train", "dropout", "s", "workspace", "workspace_bytes", "stream"]
FC_BWD = ["batch", "features", "width", "z", "fc", "s", "ds", "state", "train", "dropout", "dz", "dfc", "workspace",
          "workspace_bytes", "stream"]
FC_ENTRY = {"bsarec_caser_fc_fwd": FC_FWD, "bsarec_caser_fc_bwd": FC_BWD}
FC_PTRS16 = {"bsarec_caser_fc_fwd": ["z", "fc", "s", "workspace"],
             "bsarec_caser_fc_bwd": ["z", "fc", "s", "ds", "dz", "dfc", "workspace"]}
FC_BAD_SHAPES = [(0, 40, 36), (65537, 40, 36), (8, 0, 36), (8, 2, 36), (8, 42, 36), (8, 12292, 36), (8, 40, 0), (8, 40, 6),
                 (8, 40, 260)]
FC_CASES = [(n, dict(shape=s)) for n in FC_ENTRY for s in FC_BAD_SHAPES]
FC_CASES += [(n, dict(dropout=v)) for n in FC_ENTRY for v in (-0.1, 1.0, 1.5, float("nan"))]
FC_CASES += [(n, {p: v}) for n in FC_ENTRY for p in FC_PTRS16[n] for v in (None, "p+4")]
FC_CASES += [(n, dict(state=v)) for n in FC_ENTRY for v in (None, "p+4")]
FC_CASES += [(n, dict(workspace_bytes=v)) for n in FC_ENTRY for v in (0, "short")]


@pytest.mark.parametrize("name,change", FC_CASES, ids=A.ids(FC_CASES, "bsarec_caser_"))
def test_invalid_fc_arguments_return_negative_without_a_gpu(name, change):
    from bsarec_amd import _lib
    lib = _lib.load()
    buf = (C.c_byte * 4096)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16
    need = lib.bsarec_caser_fc_workspace_bytes(8, 40, 36)
    kw = dict(batch=8, features=40, width=36, z=p, fc=p, s=p, ds=p, state=p, train=1, dropout=0.5, dz=p, dfc=p, workspace=p,
              workspace_bytes=need, stream=None)
    for k, v in change.items():
        if k == "shape":
            kw["batch"], kw["features"], kw["width"] = v
            kw["workspace_bytes"] = 1 << 40                   # large enough for any shape: the shape itself is refused
        else:
            kw[k] = {"p+4": p + 4, "short": need - 1}.get(v, v) if isinstance(v, str) else v
    assert getattr(lib, name)(*[kw[k] for k in FC_ENTRY[name]]) < 0


def _args(**kw):
    a = argparse.Namespace(item_size=50, hidden_size=16, max_seq_length=12, hidden_dropout_prob=0.5, initializer_range=0.02,
                           caser_nh=8, caser_nv=3)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_command_line_flag():
    A.check_flag("caser_step", "Caser")


def test_mode_switch_and_fc1_views_on_the_host():
    from bsarec_amd import CaserModel
    assert CaserModel.torch_optim is True
    torch.manual_seed(4)
    default = CaserModel(_args())
    torch.manual_seed(4)
    torch_mode = CaserModel(_args(caser_step="torch"))
    torch.manual_seed(4)
    fused = CaserModel(_args(caser_step="fused"))
    assert default.caser_step == torch_mode.caser_step == "torch" and default.torch_optim is True and torch_mode.torch_optim is True
    assert fused.caser_step == "fused" and fused.torch_optim is False and fused.needs_negatives is True
    # the same keys, shapes and initial values in every mode
    assert list(fused.state_dict()) == list(default.state_dict())
    for k, v in default.state_dict().items():
        assert torch.equal(v, fused.state_dict()[k]) and torch.equal(v, torch_mode.state_dict()[k]), k
    # fused: fc1.weight and fc1.bias are views of one flat tensor, weight then bias; default: nn.Linear's own tensors
    w, b, flat = fused.fc1.weight, fused.fc1.bias, fused._fc_flat
    assert flat.numel() == w.numel() + b.numel() and flat.data_ptr() % 16 == 0
    assert w.data_ptr() == flat.data_ptr() and b.data_ptr() == flat.data_ptr() + 4 * w.numel()
    assert default._fc_flat is None
    with torch.no_grad():
        fused.fc1.bias.add_(1.0)
    assert torch.equal(flat[w.numel():], fused.fc1.bias.detach())
    # a parameter given a storage of its own is taken back, values kept; a state_dict loads in place
    with torch.no_grad():
        fused.fc1.weight.data = fused.fc1.weight.data.clone()
    fused.reflatten()
    assert fused._fc_flat is not flat and fused.fc1.weight.data_ptr() == fused._fc_flat.data_ptr()
    assert torch.equal(fused.fc1.weight.detach(), default.fc1.weight.detach())
    flat = fused._fc_flat
    fused.load_state_dict(default.state_dict())
    assert fused._fc_flat is flat and fused.fc1.bias.data_ptr() == flat.data_ptr() + 4 * w.numel()
    assert torch.equal(flat[w.numel():], default.fc1.bias.detach())
    with pytest.raises(ValueError, match="caser_step"):
        CaserModel(_args(caser_step="bogus"))
    ids = torch.randint(1, 50, (3, 12))
    with pytest.raises(RuntimeError, match="torch.optim.Adam"):
        default.train_step(ids, ids[:, 0], ids[:, 1])
    with pytest.raises(RuntimeError, match="MI355X"):               # no CPU path for the fused step either
        fused.train_step(ids, ids[:, 0], ids[:, 1])
    with pytest.raises(RuntimeError, match="MI355X"):
        fused.loss_and_grads(ids, ids[:, 0], ids[:, 1])
    with pytest.raises(RuntimeError, match="caser_step"):
        default.loss_and_grads(ids, ids[:, 0], ids[:, 1])
