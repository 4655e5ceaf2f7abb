"""Caser on the CPU: the fp64 restatement (caser_ref) against torch autograd of the Conv2d / max_pool1d / Linear / BPR formulation
in double, the padded flat layout, the state_dict round trip with a plain torch Caser, the host-only limits of the C entries, the
tie rule on a padded batch, the exported symbols, the command-line flags and what the model refuses without a GPU."""
import argparse
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.nn.functional as F  # noqa: E402

import caser_ref as R  # noqa: E402

GATE = 1e-12
GOOD = dict(batch=8, seq_len=12, width=16, n_h=8, n_v=3)
FIELDS = ("batch", "seq_len", "width", "n_h", "n_v")
BAD_CFG = [dict(batch=0), dict(batch=65537), dict(seq_len=0), dict(seq_len=257), dict(width=0), dict(width=6), dict(width=260),
           dict(n_h=0), dict(n_h=12), dict(n_h=64), dict(n_v=0), dict(n_v=17)]


def _args(**kw):
    a = argparse.Namespace(item_size=50, hidden_size=16, max_seq_length=12, hidden_dropout_prob=0.5, initializer_range=0.02,
                           caser_nh=8, caser_nv=3)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


class TorchConv(torch.nn.Module):
    """The torch block the contract names: Conv2d's under the names of CaserConv's parameters."""

    def __init__(self, L, d, nh, nv):
        super().__init__()
        self.conv_v = torch.nn.Conv2d(1, nv, (L, 1))
        self.conv_h = torch.nn.ModuleList(torch.nn.Conv2d(1, nh, (i + 1, d)) for i in range(L))

    def forward(self, x):
        x = x.unsqueeze(1)
        out_v = self.conv_v(x).reshape(x.shape[0], -1)                                   # [B, n_v d], index c d + j
        out_h = []
        for conv in self.conv_h:
            c = torch.relu(conv(x).squeeze(3))                                           # [B, n_h, L - i]
            out_h.append(F.max_pool1d(c, c.shape[2]).squeeze(2))
        return torch.cat([out_v] + out_h, 1)


class Twin(torch.nn.Module):
    def __init__(self, V, L, d, nh, nv):
        super().__init__()
        self.item_embeddings = torch.nn.Embedding(V, d)
        self.conv = TorchConv(L, d, nh, nv)
        self.fc1 = torch.nn.Linear(nv * d + nh * L, d)


def _torch_block(flat, L, d, nh, nv):
    m = TorchConv(L, d, nh, nv).double()
    w = R.split_weights(np.asarray(flat, np.float64), L, d, nh, nv)
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(torch.from_numpy(np.ascontiguousarray(w[k])).reshape(p.shape))
    return m


@pytest.mark.parametrize("shape", [(3, 5, 8, 4, 2), (2, 12, 16, 8, 3)], ids=["3-5-8-4-2", "2-12-16-8-3"])
def test_reference_equals_torch_autograd_in_double(shape):
    B, L, d, nh, nv = shape
    x, flat = R.random_case(shape)
    rng = np.random.default_rng(5)
    Fz = nv * d + nh * L
    fc_w, fc_b = rng.normal(0, 0.3, (d, Fz)), rng.normal(0, 0.3, d)
    dz = rng.normal(0, 1, (B, Fz))
    z, cache = R.forward(x, flat, nh, nv)
    dx, dflat = R.backward(cache, dz)

    m = _torch_block(flat, L, d, nh, nv)
    tx = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    tz = m(tx)
    tz.backward(torch.from_numpy(dz))
    assert np.abs(tz.detach().numpy() - z).max() <= GATE
    assert np.abs(tx.grad.numpy() - dx).max() <= GATE
    g = R.split_weights(dflat, L, d, nh, nv)
    for k, p in m.named_parameters():
        assert np.abs(p.grad.numpy().reshape(g[k].shape) - g[k]).max() <= GATE, k
    lay, total = R.layout(L, d, nh, nv)
    covered = np.zeros(total, bool)
    for name, off, shp in lay:
        covered[off:off + int(np.prod(shp))] = True
    assert not dflat[~covered].any()                                                     # zeros in the gaps

    # the whole model: lookup, block, dropout mask, fc1 + ReLU, BPR
    V = 11
    E = rng.normal(0, 1, (V, d))
    ids, pos, neg = rng.integers(0, V, (B, L)), rng.integers(1, V, B), rng.integers(1, V, B)
    keep = (rng.random((B, Fz)) < 0.7).astype(np.float64)
    loss, s, grads = R.model_loss_grads(E, flat, fc_w, fc_b, ids, pos, neg, nh, nv, keep, 0.3)
    tE = torch.from_numpy(E).requires_grad_(True)
    lin = torch.nn.Linear(Fz, d).double()
    with torch.no_grad():
        lin.weight.copy_(torch.from_numpy(fc_w))
        lin.bias.copy_(torch.from_numpy(fc_b))
    m.zero_grad()
    ts = torch.relu(lin(m(tE[torch.from_numpy(ids)]) * torch.from_numpy(keep) / 0.7))
    diff = (ts * tE[torch.from_numpy(pos)]).sum(-1) - (ts * tE[torch.from_numpy(neg)]).sum(-1)
    tl = -torch.log(torch.sigmoid(diff) + 1e-10).mean()
    tl.backward()
    assert abs(tl.item() - loss) <= GATE and np.abs(ts.detach().numpy() - s).max() <= GATE
    assert np.abs(tE.grad.numpy() - grads["item_embeddings.weight"]).max() <= GATE
    assert np.abs(lin.weight.grad.numpy() - grads["fc1.weight"]).max() <= GATE
    assert np.abs(lin.bias.grad.numpy() - grads["fc1.bias"]).max() <= GATE
    g = R.split_weights(grads["conv"], L, d, nh, nv)
    for k, p in m.named_parameters():
        assert np.abs(p.grad.numpy().reshape(g[k].shape) - g[k]).max() <= GATE, k


def test_bpr_reference_equals_autograd():
    rng = np.random.default_rng(2)
    s, p, n = (rng.normal(0, 1, (6, 8)) for _ in range(3))
    loss, ds, dp, dn = R.bpr(s, p, n)
    ts, tp, tn = (torch.from_numpy(v).requires_grad_(True) for v in (s, p, n))
    tl = -torch.log(torch.sigmoid((ts * tp).sum(-1) - (ts * tn).sum(-1)) + 1e-10).mean()
    tl.backward()
    assert abs(tl.item() - loss) <= GATE
    for a, b in ((ds, ts), (dp, tp), (dn, tn)):
        assert np.abs(a - b.grad.numpy()).max() <= GATE


@pytest.mark.parametrize("shape", [(1, 4, 4, 1), (5, 8, 4, 3), (12, 16, 8, 3), (50, 64, 16, 4), (7, 100, 8, 5), (256, 16, 4, 1),
                                   (20, 256, 32, 16)], ids=lambda s: "-".join(map(str, s)))
def test_flat_layout_offsets_alignment_and_weight_floats(shape):
    from bsarec_amd import _lib
    from bsarec_amd.caser import caser_layout
    L, d, nh, nv = shape
    lay, total = R.layout(L, d, nh, nv)
    off = 0
    for name, o, shp in lay:
        assert o % 4 == 0 and off <= o < off + 4, name                                   # 16-byte aligned, the smallest such offset
        off = o + int(np.prod(shp))
    assert total % 4 == 0 and off <= total < off + 4
    assert [n for n, _, _ in lay][:4] == ["conv_v.weight", "conv_v.bias", "conv_h.0.weight", "conv_h.0.bias"]
    assert lay[1][1] == (nv * L + 3) // 4 * 4 and lay[2][1] == lay[1][1] + (nv + 3) // 4 * 4
    assert _lib.load().bsarec_caser_weight_floats(_lib.CaserConfig(3, L, d, nh, nv)) == total
    slices, ptotal = caser_layout(L, d, nh, nv)
    assert ptotal == total and [(k, v[0]) for k, v in slices.items()] == [(n, o) for n, o, _ in lay]
    w = {n: np.full(shp, i + 1.0) for i, (n, _, shp) in enumerate(lay)}
    flat = R.flat_weights(w, L, d, nh, nv)
    back = R.split_weights(flat, L, d, nh, nv)
    assert all(np.array_equal(back[n], w[n]) for n in w) and np.count_nonzero(flat) == sum(v.size for v in w.values())


def test_state_dict_keys_init_and_round_trip_with_a_plain_torch_caser():
    from bsarec_amd import CaserModel
    V, L, d, nh, nv = 50, 12, 16, 8, 3
    torch.manual_seed(3)
    m = CaserModel(_args())
    want = [("item_embeddings.weight", (V, d)), ("conv.conv_v.weight", (nv, 1, L, 1)), ("conv.conv_v.bias", (nv,))]
    for i in range(L):
        want += [(f"conv.conv_h.{i}.weight", (nh, 1, i + 1, d)), (f"conv.conv_h.{i}.bias", (nh,))]
    want += [("fc1.weight", (d, nv * d + nh * L)), ("fc1.bias", (d,))]
    sd = m.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == want
    assert [k for k, _ in m.named_parameters()] == [k for k, _ in want]
    assert not sd["fc1.bias"].any() and abs(sd["fc1.weight"].std().item() - 0.02) < 2e-3
    for i in (0, 5, 11):                                                                 # Conv2d's default: U(+-1/sqrt(fan_in))
        b = 1 / np.sqrt((i + 1) * d)
        w = sd[f"conv.conv_h.{i}.weight"]
        assert w.abs().max().item() <= b and abs(w.std().item() - b / np.sqrt(3)) < 0.15 * b
        assert sd[f"conv.conv_h.{i}.bias"].abs().max().item() <= b
    assert sd["conv.conv_v.weight"].abs().max().item() <= 1 / np.sqrt(L)
    # the filters are views of ONE flat tensor in the padded layout of the C ABI
    flat = m.conv._flat
    lay, total = R.layout(L, d, nh, nv)
    assert flat.numel() == total
    params = dict(m.named_parameters())
    for name, off, shp in lay:
        assert params["conv." + name].data_ptr() == flat.data_ptr() + 4 * off, name

    twin = Twin(V, L, d, nh, nv)
    twin.load_state_dict(sd, strict=True)
    for k, v in sd.items():
        assert torch.equal(twin.state_dict()[k], v), k
    torch.manual_seed(5)
    other = Twin(V, L, d, nh, nv)
    m.load_state_dict(other.state_dict(), strict=True)
    for k, v in other.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k
    assert m.conv._flat is flat                                                          # loaded in place: the views still alias it
    o = dict((n, o) for n, o, _ in lay)["conv_h.4.bias"]
    assert torch.equal(flat[o:o + nh], other.conv.conv_h[4].bias.detach())
    # the twin computes what the reference computes from the flat array
    x = torch.randn(2, L, d)
    z, _ = R.forward(x.numpy(), flat.numpy(), nh, nv)
    assert np.abs(other.conv(x).detach().numpy() - z).max() < 1e-5
    # defaults when the flags are absent
    a = _args()
    del a.caser_nh, a.caser_nv
    assert (CaserModel(a).conv.n_h, CaserModel(a).conv.n_v) == (16, 4)


def _cfg(**kw):
    from bsarec_amd import _lib
    c = dict(GOOD)
    c.update(kw)
    return _lib.CaserConfig(*[c[k] for k in FIELDS])


@pytest.mark.parametrize("change", BAD_CFG, ids=["-".join(f"{k}={v}" for k, v in c.items()) for c in BAD_CFG])
def test_host_queries_reject_every_limit(change):
    from bsarec_amd import _lib
    lib = _lib.load()
    assert lib.bsarec_caser_workspace_bytes(_cfg(), 1) >= 8 * 12 * 8 * 4 and lib.bsarec_caser_workspace_bytes(_cfg(), 0) > 0
    assert lib.bsarec_caser_workspace_bytes(_cfg(), 0) < lib.bsarec_caser_workspace_bytes(_cfg(), 1)
    assert lib.bsarec_caser_weight_floats(_cfg()) == R.weight_floats(12, 16, 8, 3)
    for ok in (dict(batch=65536), dict(seq_len=256, width=256, n_h=32, n_v=16), dict(seq_len=1, width=4, n_h=4, n_v=1)):
        assert lib.bsarec_caser_workspace_bytes(_cfg(**ok), 1) > 0 and lib.bsarec_caser_weight_floats(_cfg(**ok)) > 0
    assert lib.bsarec_caser_workspace_bytes(_cfg(**change), 1) < 0
    assert lib.bsarec_caser_workspace_bytes(_cfg(**change), 0) < 0
    assert lib.bsarec_caser_weight_floats(_cfg(**change)) < 0
    assert lib.bsarec_caser_workspace_bytes(None, 1) < 0 and lib.bsarec_caser_weight_floats(None) < 0


ENTRY = {"bsarec_caser_fwd": ["cfg", "x", "weights", "train", "z", "workspace", "workspace_bytes", "stream"],
         "bsarec_caser_bwd": ["cfg", "x", "weights", "dz", "workspace", "workspace_bytes", "dx", "dweights", "stream"]}
PTRS = {"bsarec_caser_fwd": ["x", "weights", "z", "workspace"],
        "bsarec_caser_bwd": ["x", "weights", "dz", "workspace", "dx", "dweights"]}
CASES = ([(n, c) for n in ENTRY for c in BAD_CFG] + [(n, {p: v}) for n in ENTRY for p in PTRS[n] for v in (None, "p+4")] +
         [(n, dict(workspace_bytes=v)) for n in ENTRY for v in (0, "short")] + [(n, dict(cfg=None)) for n in ENTRY])


@pytest.mark.parametrize("name,change", CASES, ids=[f"{n[13:]}-{'-'.join(f'{k}={v}' for k, v in c.items())}" for n, c in CASES])
def test_invalid_arguments_return_negative_without_a_gpu(name, change):
    from bsarec_amd import _lib
    lib = _lib.load()
    buf = (C.c_byte * 4096)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16           # a 16-byte aligned host address (never dereferenced)
    need = lib.bsarec_caser_workspace_bytes(_cfg(), 1)
    kw = dict(cfg=_cfg(), x=p, weights=p, train=1, z=p, dz=p, workspace=p, workspace_bytes=need, dx=p, dweights=p, stream=None)
    for k, v in change.items():
        if k in GOOD:
            kw["cfg"] = _cfg(**{k: v})
        else:
            kw[k] = {"p+4": p + 4, "short": need - 1}.get(v, v) if isinstance(v, str) else v
    assert getattr(lib, name)(*[kw[k] for k in ENTRY[name]]) < 0


def test_symbols_are_exported_and_bound():
    from bsarec_amd import _lib
    lib = _lib.load()
    for name in ("bsarec_caser_weight_floats", "bsarec_caser_workspace_bytes", "bsarec_caser_fwd", "bsarec_caser_bwd"):
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes == _lib.EXPORTS[name][1]
    assert lib.bsarec_abi_version() == 10 and _lib.ABI_VERSION == 10                    # additive entries: the version stays


def padded_case():
    """Left-padded ids (7, 11 and 0 leading zeros) and one constant row at L = 12, d = 8: x = E[ids] repeats rows, so windows repeat
    bit for bit.  Returns (ids, x fp32, flat fp32) for (B, L, d, n_h, n_v) = (4, 12, 8, 4, 2)."""
    rng = np.random.default_rng(12)
    L, d, V = 12, 8, 30
    E = rng.normal(0, 1, (V, d)).astype(np.float32)
    ids = rng.integers(1, V, (4, L))
    ids[0, :7] = 0
    ids[1, :11] = 0
    ids[3, :] = 5
    _, flat = R.random_case((4, L, d, 4, 2))
    return ids, E[ids], flat


def test_tie_rule_on_a_padded_batch():
    ids, x, flat = padded_case()
    B, L, d, nh, nv = 4, 12, 8, 4, 2
    z, cache = R.forward(x, flat, nh, nv)
    tstar, passes, cs = cache[2], cache[3], cache[4]
    tied_positive = 0
    for h in range(1, L + 1):
        c = cs[h - 1]
        m = c.max(-1)
        ties = (m[..., None] - c <= R.TIE).sum(-1)
        tied_positive += int(((ties > 1) & (m > 0)).sum())
        assert np.array_equal(tstar[:, h - 1], np.argmax(c, -1))                         # exact ties in fp64 too: np.argmax's rule
        # the constant row: every window is the same, so the lowest t = 0 wins everywhere
        assert not tstar[3, h - 1].any()
    assert tied_positive >= 20                                                           # ties among passing cells are common here
    # torch's CPU max-pool sends the gradient to the same windows
    dz = np.random.default_rng(1).normal(0, 1, z.shape)
    dx, dflat = R.backward(cache, dz)
    m = _torch_block(flat, L, d, nh, nv)
    tx = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    m(tx).backward(torch.from_numpy(dz))
    assert np.abs(tx.grad.numpy() - dx).max() <= GATE
    g = R.split_weights(dflat, L, d, nh, nv)
    for k, p in m.named_parameters():
        assert np.abs(p.grad.numpy().reshape(g[k].shape) - g[k]).max() <= GATE, k
    # a cell at max <= 0 passes nothing
    assert np.array_equal(passes, z[:, nv * d:].reshape(B, L, nh) > 0)


def test_command_line_flags():
    from bsarec_amd.main import parse_args
    a = parse_args([])
    assert not hasattr(a, "caser_nh") and not hasattr(a, "caser_nv")                     # absent unless given
    a = parse_args(["--model_type", "Caser", "--caser_nh", "32", "--caser_nv", "2"])
    assert a.model_type == "Caser" and a.caser_nh == 32 and a.caser_nv == 2
    with pytest.raises(SystemExit):
        parse_args(["--caser_nh", "12"])


def test_model_dict_export_and_no_cpu_path():
    import bsarec_amd
    from bsarec_amd.main import MODEL_DICT
    from bsarec_amd.model import MODEL_DICT as model_table
    assert MODEL_DICT["caser"] is bsarec_amd.CaserModel                                  # what --model_type Caser looks up
    assert all(MODEL_DICT[k] is v for k, v in model_table.items()) and set(MODEL_DICT) == set(model_table) | {"caser"}
    m = bsarec_amd.CaserModel
    assert m.needs_negatives is True and m.needs_same_target is False and m.torch_optim is True
    m = bsarec_amd.CaserModel(_args())
    ids = torch.randint(1, 50, (3, 12))
    for call in (lambda: m(ids), lambda: m.predict(ids), lambda: m.last_hidden(ids), lambda: m.calculate_loss(ids, ids[:, 0], ids[:, 1]),
                 lambda: m.conv(torch.zeros(2, 12, 16))):
        with pytest.raises(RuntimeError, match="MI355X"):
            call()
    with pytest.raises(ValueError, match="neg_answers"):
        m.calculate_loss(ids, ids[:, 0])
    for bad in (dict(caser_nh=12), dict(caser_nv=0), dict(caser_nv=17), dict(hidden_size=6), dict(max_seq_length=257)):
        with pytest.raises(ValueError):
            bsarec_amd.CaserModel(_args(**bad))


def test_trainer_names_the_model_in_its_refusals():
    from bsarec_amd import CaserModel, GRU4RecModel
    from bsarec_amd.trainer import Trainer
    a = _args(lr=1e-3, adam_beta1=0.9, adam_beta2=0.999, weight_decay=0.0)
    m = CaserModel(_args())
    with pytest.raises(ValueError, match="^Caser: single GPU only$"):
        Trainer(m, None, None, None, a, process_group=object())
    for k, v in (("train_negatives", 8), ("train_lazy_adam", True), ("storage", "bf16")):
        with pytest.raises(ValueError, match="^Caser: " + k.replace("storage", "storage = 'bf16'")):
            Trainer(m, None, None, None, _args(**{k: v}))
    g = GRU4RecModel(argparse.Namespace(item_size=50, hidden_size=16, num_hidden_layers=1, max_seq_length=12, hidden_dropout_prob=0.0,
                                        initializer_range=0.02))
    for kw, msg in ((dict(process_group=object()), "GRU4Rec: single GPU only"),):
        with pytest.raises(ValueError, match="^" + msg + "$"):
            Trainer(g, None, None, None, a, **kw)
    want = {"train_negatives": "GRU4Rec: train_negatives does not apply (the model has its own BPR head)",
            "train_lazy_adam": "GRU4Rec: train_lazy_adam does not apply (the model steps through torch.optim.Adam)",
            "storage": "GRU4Rec: storage = 'bf16' does not apply (the GRU kernels are fp32)"}
    for k, v in (("train_negatives", 8), ("train_lazy_adam", True), ("storage", "bf16")):
        with pytest.raises(ValueError) as e:
            Trainer(g, None, None, None, _args(**{k: v}))
        assert str(e.value) == want[k]                                                   # word for word what they were
