"""The GRU stack and the GRU4Rec model on the host, no GPU: the fp64 restatement (gru_ref) against torch.nn.GRU + nn.Linear in
double, the header as plain C, the argument checks of the entry points (they return < 0 before any HIP call), the command-line
flag, MODEL_DICT, the state_dict contract against a torch twin, and the absence of a CPU path."""
import argparse
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import ROOT, rel_l2
import gru_ref as R


def _args(**kw):
    a = argparse.Namespace(item_size=301, hidden_size=64, gru_hidden_size=64, num_hidden_layers=2, max_seq_length=20,
                           hidden_dropout_prob=0.5, initializer_range=0.02)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


class Twin(torch.nn.Module):
    """The torch model the contract names: the same attribute names, so the same state_dict keys."""

    def __init__(self, V, d, H, N):
        super().__init__()
        self.item_embeddings = torch.nn.Embedding(V, d)
        self.gru_layers = torch.nn.GRU(d, H, N, bias=False, batch_first=True)
        self.dense = torch.nn.Linear(H, d)

    def forward(self, ids):
        return self.dense(self.gru_layers(self.item_embeddings(ids))[0])


@pytest.mark.parametrize("B,L,I,H,N,O", [(5, 7, 12, 32, 2, 20), (3, 1, 4, 32, 1, 0)])
def test_reference_equals_torch_gru_and_linear_in_double(B, L, I, H, N, O):
    rng = np.random.default_rng(B * 100 + L)
    x = rng.normal(0, 1, (B, L, I))
    flat = R.random_weights(rng, I, H, N, O).astype(np.float64)
    if O:
        flat[-O:] = rng.normal(0, 0.3, O)                  # a bias that is not zero
    dout = rng.normal(0, 1, (B, L, O or H))
    out, cache = R.forward(x, flat, H, N, O)
    dx, dflat = R.backward(cache, dout)

    gru = torch.nn.GRU(I, H, N, bias=False, batch_first=True).double()
    lin = torch.nn.Linear(H, O).double() if O else None
    w = R.split_weights(flat, I, H, N, O)
    with torch.no_grad():
        for k in range(N):
            getattr(gru, f"weight_ih_l{k}").copy_(torch.from_numpy(w[f"weight_ih_l{k}"]))
            getattr(gru, f"weight_hh_l{k}").copy_(torch.from_numpy(w[f"weight_hh_l{k}"]))
        if O:
            lin.weight.copy_(torch.from_numpy(w["out_weight"]))
            lin.bias.copy_(torch.from_numpy(w["out_bias"]))
    tx = torch.from_numpy(x).requires_grad_(True)
    ty = gru(tx)[0]
    tout = lin(ty) if O else ty
    tout.backward(torch.from_numpy(dout))
    assert np.abs(out - tout.detach().numpy()).max() <= 1e-12
    assert np.abs(dx - tx.grad.numpy()).max() <= 1e-12
    g = R.split_weights(dflat, I, H, N, O)
    for k in range(N):
        assert np.abs(g[f"weight_ih_l{k}"] - getattr(gru, f"weight_ih_l{k}").grad.numpy()).max() <= 1e-12
        assert np.abs(g[f"weight_hh_l{k}"] - getattr(gru, f"weight_hh_l{k}").grad.numpy()).max() <= 1e-12
    if O:
        assert np.abs(g["out_weight"] - lin.weight.grad.numpy()).max() <= 1e-12
        assert np.abs(g["out_bias"] - lin.bias.grad.numpy()).max() <= 1e-12
    # the last-position form: a gradient at L - 1 alone
    dlast = rng.normal(0, 1, (B, O or H))
    dx2, dflat2 = R.backward(cache, R.last_only_dout(dlast, L))
    tx.grad = None
    gru.zero_grad()
    (lin(gru(tx)[0]) if O else gru(tx)[0])[:, -1].backward(torch.from_numpy(dlast))
    assert np.abs(dx2 - tx.grad.numpy()).max() <= 1e-12
    assert np.abs(R.split_weights(dflat2, I, H, N, O)["weight_hh_l0"] - gru.weight_hh_l0.grad.numpy()).max() <= 1e-12


def test_bpr_reference_equals_autograd():
    rng = np.random.default_rng(5)
    s, p, n = (rng.normal(0, 1, (9, 8)) for _ in range(3))
    ts, tp, tn = (torch.from_numpy(v).requires_grad_(True) for v in (s, p, n))
    loss = -torch.log(torch.sigmoid((ts * tp).sum(-1) - (ts * tn).sum(-1)) + 1e-10).mean()
    loss.backward()
    rl, ds, dp, dn = R.bpr(s, p, n)
    assert abs(rl - loss.item()) <= 1e-12
    for a, b in ((ds, ts), (dp, tp), (dn, tn)):
        assert np.abs(a - b.grad.numpy()).max() <= 1e-12


def test_header_block_is_plain_c99_and_links(tmp_path):
    lib_dir = os.path.join(ROOT, "bsarec_amd")
    if not os.path.exists(os.path.join(lib_dir, "libbsarec_hip.so")) or not shutil.which("gcc"):
        pytest.skip("library or gcc missing")
    src = r"""
#include "bsarec_hip.h"
#include <stdio.h>
int main(void) {
    bsarec_gru_config_t cfg = {256, 50, 64, 64, 2, 64};
    long ws = bsarec_gru_workspace_bytes(&cfg, 1), ws0 = bsarec_gru_workspace_bytes(&cfg, 0), nw = bsarec_gru_weight_floats(&cfg);
    cfg.hidden_size = 48;
    printf("%d %ld %ld %ld %ld\n", bsarec_abi_version(), ws, ws0, nw, bsarec_gru_workspace_bytes(&cfg, 1));
    return (bsarec_abi_version() == 10 && ws > 0 && ws0 > 0 && ws0 < ws && bsarec_gru_workspace_bytes(&cfg, 1) < 0) ? 0 : 1;
}
"""
    f = tmp_path / "host.c"
    f.write_text(src)
    exe = tmp_path / "host"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(f), "-o", str(exe),
                    "-L", lib_dir, "-lbsarec_hip", f"-Wl,-rpath,{lib_dir}"], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ver, ws, ws0, nw, bad = (int(v) for v in r.stdout.split())
    assert ver == 10 and nw == 3 * 64 * 64 * 4 + 64 * 64 + 64


def test_symbols_are_exported_and_bound():
    from bsarec_amd import _lib
    lib = _lib.load()
    for name in ("bsarec_gru_weight_floats", "bsarec_gru_workspace_bytes", "bsarec_gru_fwd", "bsarec_gru_bwd"):
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes == _lib.EXPORTS[name][1]
    assert lib.bsarec_abi_version() == 10 and _lib.ABI_VERSION == 10


GOOD = dict(batch=8, seq_len=10, input_size=64, hidden_size=64, num_layers=2, out_size=64)
BAD_CFG = [dict(batch=0), dict(batch=-1), dict(batch=65537), dict(seq_len=0), dict(seq_len=257), dict(input_size=0),
           dict(input_size=2), dict(input_size=66), dict(input_size=260), dict(hidden_size=0), dict(hidden_size=16),
           dict(hidden_size=48), dict(hidden_size=160), dict(hidden_size=256), dict(num_layers=0), dict(num_layers=5),
           dict(out_size=2), dict(out_size=-4), dict(out_size=66), dict(out_size=260)]
FWD = ["cfg", "x", "weights", "train", "last_only", "out", "workspace", "workspace_bytes", "stream"]
BWD = ["cfg", "x", "weights", "last_only", "dout", "workspace", "workspace_bytes", "dx", "dweights", "stream"]
ENTRY = {"bsarec_gru_fwd": FWD, "bsarec_gru_bwd": BWD}
PTRS = {"bsarec_gru_fwd": ["x", "weights", "out", "workspace"],
        "bsarec_gru_bwd": ["x", "weights", "dout", "workspace", "dx", "dweights"]}
CASES = ([(n, c) for n in ENTRY for c in BAD_CFG] + [(n, {p: v}) for n in ENTRY for p in PTRS[n] for v in (None, "p+4")] +
         [(n, dict(workspace_bytes=v)) for n in ENTRY for v in (0, "short")] + [(n, dict(cfg=None)) for n in ENTRY])


def _cfg(**kw):
    from bsarec_amd import _lib
    c = dict(GOOD)
    c.update(kw)
    return _lib.GruConfig(*[c[k] for k in ("batch", "seq_len", "input_size", "hidden_size", "num_layers", "out_size")])


@pytest.mark.parametrize("change", BAD_CFG, ids=["-".join(f"{k}={v}" for k, v in c.items()) for c in BAD_CFG])
def test_workspace_query_rejects_every_limit(change):
    from bsarec_amd import _lib
    lib = _lib.load()
    assert lib.bsarec_gru_workspace_bytes(_cfg(), 1) > lib.bsarec_gru_workspace_bytes(_cfg(), 0) > 0
    assert lib.bsarec_gru_weight_floats(_cfg()) == 2 * 2 * 3 * 64 * 64 + 64 * 64 + 64
    assert lib.bsarec_gru_workspace_bytes(_cfg(out_size=0), 1) > 0            # no projection is a valid stack
    assert lib.bsarec_gru_workspace_bytes(_cfg(**change), 1) < 0
    assert lib.bsarec_gru_workspace_bytes(_cfg(**change), 0) < 0
    assert lib.bsarec_gru_weight_floats(_cfg(**change)) < 0
    assert lib.bsarec_gru_workspace_bytes(None, 1) < 0


@pytest.mark.parametrize("name,change", CASES, ids=[f"{n[11:]}-{'-'.join(f'{k}={v}' for k, v in c.items())}" for n, c in CASES])
def test_invalid_arguments_return_negative_without_a_gpu(name, change):
    from bsarec_amd import _lib
    lib = _lib.load()
    buf = (C.c_byte * 4096)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16           # a 16-byte aligned host address (never dereferenced)
    need = lib.bsarec_gru_workspace_bytes(_cfg(), 1)
    kw = dict(cfg=_cfg(), x=p, weights=p, train=1, last_only=0, out=p, dout=p, workspace=p, workspace_bytes=need, dx=p,
              dweights=p, stream=None)
    for k, v in change.items():
        if k in GOOD:
            kw["cfg"] = _cfg(**{k: v})
        else:
            kw[k] = {"p+4": p + 4, "short": need - 1}.get(v, v) if isinstance(v, str) else v
    assert getattr(lib, name)(*[kw[k] for k in ENTRY[name]]) < 0


def test_command_line_flag():
    from bsarec_amd.main import parse_args
    assert not hasattr(parse_args([]), "gru_hidden_size")          # absent unless given: the logged arguments stay as they were
    a = parse_args(["--model_type", "GRU4Rec", "--gru_hidden_size", "96"])
    assert a.model_type == "GRU4Rec" and a.gru_hidden_size == 96
    with pytest.raises(SystemExit):
        parse_args(["--gru_hidden_size", "100"])


def test_model_dict_and_export():
    import bsarec_amd
    from bsarec_amd.model import MODEL_DICT
    assert MODEL_DICT["gru4rec"] is bsarec_amd.GRU4RecModel
    assert set(MODEL_DICT) == {"bsarec", "sasrec", "fmlprec", "duorec", "gru4rec"}
    m = bsarec_amd.GRU4RecModel
    assert m.needs_negatives is True and m.needs_same_target is False and m.torch_optim is True


@pytest.mark.parametrize("H,N", [(64, 2), (96, 1), (128, 3)])
def test_state_dict_keys_shapes_and_init(H, N):
    from bsarec_amd import GRU4RecModel
    V, d = 301, 64
    torch.manual_seed(3)
    m = GRU4RecModel(_args(gru_hidden_size=H, num_hidden_layers=N))
    want = [("item_embeddings.weight", (V, d))]
    for k in range(N):
        want += [(f"gru_layers.weight_ih_l{k}", (3 * H, d if k == 0 else H)), (f"gru_layers.weight_hh_l{k}", (3 * H, H))]
    want += [("dense.weight", (d, H)), ("dense.bias", (d,))]
    sd = m.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == want
    assert [k for k, _ in m.named_parameters()] == [k for k, _ in want]
    assert not sd["dense.bias"].any()
    assert abs(sd["item_embeddings.weight"].std().item() - 0.02) < 2e-3 and abs(sd["dense.weight"].std().item() - 0.02) < 2e-3
    w = sd["gru_layers.weight_hh_l0"]
    b = 1 / np.sqrt(H)
    assert w.abs().max().item() <= b and abs(w.std().item() - b / np.sqrt(3)) < 0.1 * b
    # the GRU and Linear parameters are views of ONE flat tensor in the order of the C ABI's weight array
    flat = m.gru_layers._flat
    off = 0
    for k, shp in want[1:]:
        p = dict(m.named_parameters())[k]
        assert p.data_ptr() == flat.data_ptr() + 4 * off, k
        off += int(np.prod(shp))
    assert off == flat.numel()
    assert getattr(_args(), "gru_hidden_size") == 64 and GRU4RecModel(argparse.Namespace(
        item_size=10, hidden_size=8, num_hidden_layers=1, max_seq_length=5, hidden_dropout_prob=0.0,
        initializer_range=0.02)).gru_layers.hidden_size == 64                 # the default


def test_torch_twin_loads_the_state_dict_and_the_reverse():
    from bsarec_amd import GRU4RecModel
    V, d, H, N = 301, 64, 96, 2
    torch.manual_seed(4)
    m = GRU4RecModel(_args(gru_hidden_size=H))
    twin = Twin(V, d, H, N)
    twin.load_state_dict(m.state_dict(), strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(twin.state_dict()[k], v), k
    torch.manual_seed(5)
    other = Twin(V, d, H, N)
    flat_before = m.gru_layers._flat
    m.load_state_dict(other.state_dict(), strict=True)
    for k, v in other.state_dict().items():
        assert torch.equal(m.state_dict()[k], v), k
    assert m.gru_layers._flat is flat_before                      # loaded in place: the views still alias the flat array
    assert torch.equal(m.gru_layers._flat[:3 * H * d].view(3 * H, d), other.gru_layers.weight_ih_l0.detach())
    assert torch.equal(m.gru_layers._flat[-d:], other.dense.bias.detach())


def test_no_cpu_path():
    from bsarec_amd import GRU4RecModel
    m = GRU4RecModel(_args())
    ids = torch.randint(1, 301, (3, 20))
    with pytest.raises(RuntimeError, match="MI355X"):
        m(ids)
    with pytest.raises(RuntimeError, match="MI355X"):
        m.last_hidden(ids)
    with pytest.raises(RuntimeError, match="MI355X"):
        m.calculate_loss(ids, ids[:, 0], ids[:, 1])
    with pytest.raises(ValueError, match="neg_answers"):
        m.calculate_loss(ids, ids[:, 0])
    with pytest.raises(RuntimeError, match="MI355X"):
        m.gru_layers(torch.zeros(2, 5, 64))
    with pytest.raises(ValueError):
        GRU4RecModel(_args(gru_hidden_size=48))


def test_trainer_refuses_what_gru4rec_has_not():
    from bsarec_amd import GRU4RecModel
    from bsarec_amd.trainer import Trainer
    m = GRU4RecModel(_args())
    a = _args(lr=1e-3, adam_beta1=0.9, adam_beta2=0.999, weight_decay=0.0)
    with pytest.raises(ValueError, match="GRU4Rec: single GPU only"):
        Trainer(m, None, None, None, a, process_group=object())
    for k, v in (("train_negatives", 8), ("train_lazy_adam", True), ("storage", "bf16")):
        with pytest.raises(ValueError, match="GRU4Rec"):
            Trainer(m, None, None, None, _args(**{k: v}, lr=1e-3, adam_beta1=0.9, adam_beta2=0.999, weight_decay=0.0))
