"""The personalised Caser (args.caser_user) on the host, no GPU: the fp64 restatement (caser_user_ref) against torch autograd and
torch.optim.Adam in double on a twin module, the state_dict in both directions, the default model's unchanged keys, the new symbols
and their bindings, the header as plain C, the argument limits of the entry points (they return < 0 before any HIP call), the
model's refusals, the fc2 views and the command-line flag."""
import argparse
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import abi_cases as A  # noqa: E402
import caser_step_ref as S  # noqa: E402
import caser_user_ref as UR  # noqa: E402
from test_caser_cpu import TorchConv  # noqa: E402

V, U, D, L, B, NH, NV = 23, 4, 8, 5, 6, 4, 2
FZ = NV * D + NH * L


class TwinUser(torch.nn.Module):
    """The torch module the contract names: the modules of CaserModel with caser_user, in the state_dict's order."""

    def __init__(self, V, U, L, d, nh, nv):
        super().__init__()
        self.item_embeddings = torch.nn.Embedding(V, d)
        self.user_embeddings = torch.nn.Embedding(U, d)
        self.conv = TorchConv(L, d, nh, nv)
        self.fc1 = torch.nn.Linear(nv * d + nh * L, d)
        self.fc2 = torch.nn.Linear(2 * d, d)

    def state(self, ids, users, mult=None):
        z = self.conv(self.item_embeddings(ids))
        z1 = torch.relu(self.fc1(z if mult is None else z * mult))
        return torch.relu(self.fc2(torch.cat([z1, self.user_embeddings(users)], -1)))

    def loss(self, ids, users, pos, neg, mult=None):
        E, s = self.item_embeddings, self.state(ids, users, mult)
        return -torch.log(torch.sigmoid((s * E(pos)).sum(-1) - (s * E(neg)).sum(-1)) + 1e-10).mean()


def _batch():
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(1, V, (B, L), generator=g)
    ids[:2, :2] = 0
    pos = torch.randint(1, V, (B,), generator=g)
    neg = torch.randint(1, V, (B,), generator=g)
    pos[0], neg[1] = ids[0, -1], ids[1, -1]               # rows that the lookup and the head both touch
    neg[2] = pos[2]                                       # a row whose head terms cancel
    users = torch.tensor([0, 2, 2, 3, 0, 2])              # id 0, U - 1, repeats; user 1 is named by no row
    return ids, users, pos, neg


def _twin():
    torch.manual_seed(9)
    twin = TwinUser(V, U, L, D, NH, NV).double()
    with torch.no_grad():
        twin.item_embeddings.weight.mul_(0.8)
        twin.fc1.bias.normal_(0.0, 0.1)
        twin.fc2.bias.normal_(0.0, 0.1)
    return twin


@pytest.mark.parametrize("wd", [0.0, 0.01])
def test_reference_equals_autograd_and_torch_adam_in_double(wd):
    twin = _twin()
    assert [k for k, _ in twin.named_parameters()] == UR.keys(L)
    params = {k: p.detach().numpy().copy() for k, p in twin.named_parameters()}
    ids, users, pos, neg = _batch()
    opt = torch.optim.Adam(twin.parameters(), lr=1e-2, weight_decay=wd)
    st = UR.adam_state(lr=1e-2, weight_decay=wd)
    for step in range(1, 4):
        mult = UR.dropout_mult(B, FZ, 0.5, 1234567, step)             # an explicit mask: the library's stream at this step
        rloss, out, rgrads = UR.loss_and_grads(params, ids.numpy(), users.numpy(), pos.numpy(), neg.numpy(), mult)
        assert (out["s"] > 0).any() and (out["s"] == 0).any() and (out["z1"] == 0).any()      # both ReLUs take both branches
        assert np.array_equal(out["x2"][:, D:], params["user_embeddings.weight"][users.numpy()])
        opt.zero_grad()
        loss = twin.loss(ids, users, pos, neg, torch.from_numpy(mult))
        loss.backward()
        assert abs(rloss - loss.item()) <= 1e-12
        assert np.abs(out["s"] - twin.state(ids, users, torch.from_numpy(mult)).detach().numpy()).max() <= 1e-12
        for k, p in twin.named_parameters():
            assert rgrads[k].shape == tuple(p.shape)
            assert np.abs(rgrads[k] - p.grad.numpy()).max() <= 1e-12, (step, k)
        assert not rgrads["user_embeddings.weight"][1].any() and rgrads["user_embeddings.weight"][2].any()
        opt.step()
        assert UR.train_step(params, st, ids.numpy(), users.numpy(), pos.numpy(), neg.numpy(), mult) == rloss
        for k, p in twin.named_parameters():
            assert np.abs(params[k] - p.detach().numpy()).max() <= 1e-12, (step, k)
    assert st.t == 3


def test_reference_drops_a_user_id_outside_the_table():
    twin = _twin()
    params = {k: p.detach().numpy().copy() for k, p in twin.named_parameters()}
    ids, users, pos, neg = (t.numpy() for t in _batch())
    out_of_range = users.copy()
    out_of_range[1], out_of_range[3] = U, -1
    _, out, g = UR.loss_and_grads(params, ids, out_of_range, pos, neg)
    assert not out["x2"][[1, 3], D:].any() and out["x2"][0, D:].any()
    # the same as a table with a zero row behind it that gets no gradient
    wide = dict(params)
    wide["user_embeddings.weight"] = np.concatenate([params["user_embeddings.weight"], np.zeros((1, D))])
    moved = np.where((out_of_range < 0) | (out_of_range >= U), U, out_of_range)
    lw, _, gw = UR.loss_and_grads(wide, ids, moved, pos, neg)
    assert np.array_equal(g["user_embeddings.weight"], gw["user_embeddings.weight"][:U])
    assert np.array_equal(g["fc2.weight"], gw["fc2.weight"])


def _args(**kw):
    a = argparse.Namespace(item_size=V, hidden_size=D, max_seq_length=L, hidden_dropout_prob=0.5, initializer_range=0.02,
                           caser_nh=NH, caser_nv=NV, num_users=U)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


@pytest.mark.parametrize("mode", ["torch", "fused"])
def test_state_dict_loads_both_ways_and_the_default_keeps_its_keys(mode):
    from bsarec_amd import CaserModel
    twin = _twin().float()
    torch.manual_seed(2)
    m = CaserModel(_args(caser_user=True, caser_step=mode))
    assert m.needs_user_ids is True and CaserModel.needs_user_ids is False
    assert list(m.state_dict()) == list(twin.state_dict()) == UR.keys(L)
    for k, v in twin.state_dict().items():
        assert tuple(m.state_dict()[k].shape) == tuple(v.shape), k
    assert tuple(m.user_embeddings.weight.shape) == (U, D) and tuple(m.fc2.weight.shape) == (D, 2 * D)
    assert not m.fc2.bias.any() and 0.005 < m.fc2.weight.std().item() < 0.04 and 0.005 < m.user_embeddings.weight.std().item() < 0.04
    m.load_state_dict(twin.state_dict())
    for k, v in twin.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k
    other = TwinUser(V, U, L, D, NH, NV)
    other.load_state_dict(m.state_dict())
    for k, v in m.state_dict().items():
        assert torch.equal(other.state_dict()[k], v), k
    # the default model: today's keys, and the draws of its init are not moved by the flag's code
    torch.manual_seed(2)
    off = CaserModel(_args(caser_step=mode))
    torch.manual_seed(2)
    off2 = CaserModel(_args(caser_step=mode, caser_user=False))
    assert off.needs_user_ids is False and off.caser_user is False
    assert list(off.state_dict()) == list(off2.state_dict()) == S.keys(L)
    assert not hasattr(off, "user_embeddings") and not hasattr(off, "fc2") and off._fc2_flat is None
    for k, v in off.state_dict().items():
        assert torch.equal(v, off2.state_dict()[k]), k


def test_refusals():
    from bsarec_amd import CaserModel
    for bad in (dict(num_users=0), dict(num_users=-3), dict(num_users=None)):
        with pytest.raises(ValueError, match="num_users"):
            CaserModel(_args(caser_user=True, **bad))
    a = _args(caser_user=True)
    del a.num_users
    with pytest.raises(ValueError, match="num_users"):
        CaserModel(a)
    CaserModel(_args(num_users=0))                                   # not read without the flag
    ids = torch.randint(1, V, (B, L))
    u = torch.arange(B, dtype=torch.int32) % U
    for mode in ("torch", "fused"):
        m = CaserModel(_args(caser_user=True, caser_step=mode))
        calls = [lambda x: m(ids, x), lambda x: m.predict(ids, x), lambda x: m.last_hidden(ids, x),
                 lambda x: m.calculate_loss(ids, ids[:, 0], ids[:, 1], user_ids=x)]
        if mode == "fused":
            calls += [lambda x: m.train_step(ids, ids[:, 0], ids[:, 1], user_ids=x),
                      lambda x: m.loss_and_grads(ids, ids[:, 0], ids[:, 1], user_ids=x)]
        for call in calls:                                           # the refusal stands before the device check
            with pytest.raises(ValueError, match="needs user_ids"):
                call(None)
            for shape in ((B + 1,), (B, 2), (1, B), (B, 1, 1), ()):
                with pytest.raises(ValueError, match="user_ids must be"):
                    call(torch.zeros(shape, dtype=torch.int64))
            for ok in (u, u.view(B, 1)):                             # accepted: what is left is "no CPU path"
                with pytest.raises(RuntimeError, match="MI355X"):
                    call(ok)
    got = m._users(u.view(B, 1), ids)
    assert got.dtype == torch.int64 and tuple(got.shape) == (B,) and torch.equal(got, u.long())
    off = CaserModel(_args())                                        # the default model ignores user_ids, as before
    assert off._users(None, ids) is None and off._users(torch.zeros(3, 3), ids) is None
    with pytest.raises(RuntimeError, match="MI355X"):
        off(ids)


def test_fc2_views_after_reflatten():
    from bsarec_amd import CaserModel
    torch.manual_seed(4)
    fused = CaserModel(_args(caser_user=True, caser_step="fused"))
    torch.manual_seed(4)
    plain = CaserModel(_args(caser_user=True, caser_step="torch"))
    assert plain._fc2_flat is None and plain._fc_flat is None
    for k, v in plain.state_dict().items():
        assert torch.equal(v, fused.state_dict()[k]), k
    w, b, flat = fused.fc2.weight, fused.fc2.bias, fused._fc2_flat
    assert flat.numel() == w.numel() + b.numel() == 2 * D * D + D and flat.data_ptr() % 16 == 0
    assert w.data_ptr() == flat.data_ptr() and b.data_ptr() == flat.data_ptr() + 4 * w.numel()
    f1 = fused._fc_flat
    assert fused.fc1.weight.data_ptr() == f1.data_ptr() and f1.data_ptr() != flat.data_ptr()
    with torch.no_grad():
        fused.fc2.bias.add_(1.0)
    assert torch.equal(flat[w.numel():], fused.fc2.bias.detach())
    with torch.no_grad():                                            # a storage of its own is taken back, values kept
        fused.fc2.weight.data = fused.fc2.weight.data.clone()
    fused.reflatten()
    assert fused._fc2_flat is not flat and fused.fc2.weight.data_ptr() == fused._fc2_flat.data_ptr()
    assert fused._fc_flat is f1                                      # fc1's array was not the one that changed
    assert torch.equal(fused.fc2.weight.detach(), plain.fc2.weight.detach())
    flat = fused._fc2_flat
    fused.load_state_dict(plain.state_dict())                        # in place
    assert fused._fc2_flat is flat and torch.equal(flat[w.numel():], plain.fc2.bias.detach())
    fused.load_state_dict(plain.state_dict(), assign=True)           # new storages: the views are rebuilt on the next reflatten
    fused.reflatten()
    w, b = fused.fc2.weight, fused.fc2.bias
    assert w.data_ptr() == fused._fc2_flat.data_ptr() and b.data_ptr() == fused._fc2_flat.data_ptr() + 4 * w.numel()
    assert fused._fused is None


def test_command_line_flag():
    from bsarec_amd.main import MODEL_DICT, parse_args
    from bsarec_amd.model import MODEL_DICT as model_table
    assert not hasattr(parse_args([]), "caser_user")                 # absent unless given: the logged arguments stay as they were
    a = parse_args(["--model_type", "Caser", "--caser_user", "--caser_step", "fused"])
    assert a.caser_user is True and a.caser_step == "fused"
    assert parse_args(["--caser_user"]).caser_user is True and not hasattr(parse_args(["--caser_user"]), "caser_step")
    assert set(MODEL_DICT) == set(model_table) | {"caser"}


NAMES = ("bsarec_caser_fc2_floats", "bsarec_caser_user_step_workspace_bytes", "bsarec_caser_user_loss_grad",
         "bsarec_caser_user_train_step")


def test_symbols_are_exported_and_bound():
    from bsarec_amd import _lib
    A.check_symbols(NAMES, {"bsarec_caser_user_loss_grad": 21, "bsarec_caser_user_train_step": 15}, _lib.CaserUserStepConfig,
                    ["step", "num_users"], C.sizeof(_lib.CaserStepConfig) + 4)


def test_header_block_is_plain_c99_and_links(tmp_path):
    src = r"""
#include "bsarec_hip.h"
#include <stdio.h>
int main(void) {
    bsarec_caser_user_step_config_t cfg = {{{256, 50, 64, 16, 4}, 3417, 0.5f}, 6040};
    long ws = bsarec_caser_user_step_workspace_bytes(&cfg), sws = bsarec_caser_step_workspace_bytes(&cfg.step);
    long fc2 = bsarec_caser_fc2_floats(&cfg.step.conv);
    int (*lg)(const bsarec_caser_user_step_config_t *, const float *, const float *, const float *, const float *, const float *,
              const int64_t *, const int64_t *, const int64_t *, const int64_t *, void *, int, float *, float *, float *, float *,
              float *, float *, void *, long, void *) = bsarec_caser_user_loss_grad;
    int (*ts)(const bsarec_caser_user_step_config_t *, const int64_t *, const int64_t *, const int64_t *, const int64_t *,
              const bsarec_adam_t *, const bsarec_adam_t *, const bsarec_adam_t *, const bsarec_adam_t *, const bsarec_adam_t *,
              void *, float *, void *, long, void *) = bsarec_caser_user_train_step;
    long bad;
    cfg.num_users = 0;
    bad = bsarec_caser_user_step_workspace_bytes(&cfg);
    printf("%d %ld %ld %ld %ld\n", bsarec_abi_version(), ws, sws, fc2, bad);
    return (lg && ts && bsarec_abi_version() == 10 && ws > sws && sws > 0 && bad < 0) ? 0 : 1;
}
"""
    ver, ws, sws, fc2, bad = A.run_c99(tmp_path, src)
    Bq, d, Uq = 256, 64, 6040
    assert ver == 10 and fc2 == d * 2 * d + d
    assert ws == sws + 4 * (2 * Bq * d + Bq * d + Bq * d + 2 * Bq * d + 2 * Uq * d)      # x2 | s | ds | dx2 | the user accumulator


GOOD = dict(batch=8, seq_len=12, width=16, n_h=8, n_v=3, item_size=50, dropout=0.5, num_users=7)
CONV = ("batch", "seq_len", "width", "n_h", "n_v")
BAD_CFG = [dict(num_users=0), dict(num_users=-1), dict(batch=0), dict(width=6), dict(n_h=12), dict(item_size=1), dict(dropout=1.0),
           dict(dropout=float("nan"))]
LOSS_GRAD = ["cfg", "item_emb", "user_emb", "weights", "fc", "fc2", "ids", "users", "answers", "neg_answers", "state", "train",
             "loss_out", "d_item_emb", "d_user_emb", "dweights", "dfc", "dfc2", "workspace", "workspace_bytes", "stream"]
TRAIN_STEP = ["cfg", "ids", "users", "answers", "neg_answers", "adam_items", "adam_users", "adam_weights", "adam_fc", "adam_fc2",
              "state", "loss_out", "workspace", "workspace_bytes", "stream"]
ENTRY = {"bsarec_caser_user_loss_grad": LOSS_GRAD, "bsarec_caser_user_train_step": TRAIN_STEP}
PTRS16 = {"bsarec_caser_user_loss_grad": ["item_emb", "user_emb", "weights", "fc", "fc2", "d_item_emb", "d_user_emb", "dweights",
                                          "dfc", "dfc2", "workspace"],
          "bsarec_caser_user_train_step": ["workspace"]}
PTRS8 = ["ids", "users", "answers", "neg_answers", "state"]
ADAMS = ("adam_items", "adam_users", "adam_weights", "adam_fc", "adam_fc2")
# the three Adams of the item-only step are walked through in test_caser_step_cpu.py: here the two new ones, and every n
CASES = A.step_cases(ENTRY, BAD_CFG, PTRS16, PTRS8, ADAMS, adams_in_full=("adam_users", "adam_fc2"),
                     sizes=(0, "short", "item-only"),
                     hyper=[{f"{a}.{k}": v} for a in ADAMS[1:] for k, v in (("lr", 2e-3), ("beta1", 0.8), ("beta2", 0.99))] +
                     [{"adam_items.lr": 2e-3}])


def _cfg(**kw):
    from bsarec_amd import _lib
    c = dict(GOOD)
    c.update(kw)
    return _lib.CaserUserStepConfig(_lib.CaserStepConfig(_lib.CaserConfig(*[c[k] for k in CONV]), c["item_size"], c["dropout"]),
                                    c["num_users"])


def _adam_n(lib):
    conv = _cfg().step.conv
    return {"adam_items": GOOD["item_size"] * GOOD["width"], "adam_users": GOOD["num_users"] * GOOD["width"],
            "adam_weights": lib.bsarec_caser_weight_floats(conv), "adam_fc": lib.bsarec_caser_fc_floats(conv),
            "adam_fc2": lib.bsarec_caser_fc2_floats(conv)}


SPEC = A.spec(GOOD, _cfg, ENTRY, PTRS16, PTRS8, need=lambda lib: lib.bsarec_caser_user_step_workspace_bytes(_cfg()), adam_n=_adam_n,
              sizes=lambda lib: {"item-only": lib.bsarec_caser_step_workspace_bytes(_cfg().step)})


def test_workspace_and_size_queries():
    from bsarec_amd import _lib
    lib = _lib.load()
    item_only = lib.bsarec_caser_step_workspace_bytes(_cfg().step)
    Bq, d = GOOD["batch"], GOOD["width"]
    assert lib.bsarec_caser_user_step_workspace_bytes(_cfg()) == item_only + 4 * (6 * Bq * d + 2 * GOOD["num_users"] * d)
    assert lib.bsarec_caser_user_step_workspace_bytes(_cfg(num_users=1)) == item_only + 4 * (6 * Bq * d + 2 * d)
    assert lib.bsarec_caser_user_step_workspace_bytes(None) < 0
    for change in BAD_CFG:
        assert lib.bsarec_caser_user_step_workspace_bytes(_cfg(**change)) < 0, change
    assert lib.bsarec_caser_fc2_floats(_cfg().step.conv) == 2 * d * d + d
    assert lib.bsarec_caser_fc2_floats(None) < 0 and lib.bsarec_caser_fc2_floats(_cfg(width=6).step.conv) < 0


@pytest.mark.parametrize("name,change", CASES, ids=A.ids(CASES, "bsarec_caser_user_"))
def test_invalid_arguments_return_negative_without_a_gpu(name, change):
    assert A.call(SPEC, name, change) < 0
