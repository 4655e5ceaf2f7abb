"""The HIP full-catalogue cross-entropy head on the host, no GPU: the fp64 restatement (ce_head_ref) against autograd through
F.cross_entropy(h @ E.T, a), the exported symbols, the workspace bound, the argument checks of the entry points (they return
< 0 before any HIP call), and the --duorec_ce_head flag."""
import argparse
import ctypes as C
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import GOLDEN, rel_l2
import ce_head_ref as R


def _model(**kw):
    from bsarec_amd import DuoRecModel
    z = np.load(os.path.join(GOLDEN, "duorec_A_d64_L50_h2.npz"))
    cfg = json.loads(str(z["cfg"]))
    return DuoRecModel(argparse.Namespace(hidden_act="gelu", batch_size=10, c=3, **cfg, **kw))


@pytest.mark.parametrize("B,V,d", [(1, 1, 4), (2, 2, 4), (5, 37, 12), (33, 130, 12)])
def test_reference_equals_autograd_through_the_torch_head(B, V, d):
    g = 0.37
    rng = np.random.default_rng(B * 1000 + V)
    h, E = rng.normal(0, 1, (B, d)), rng.normal(0, 1, (V, d))
    a = rng.integers(0, V, B)
    a[0], a[-1] = 0, V - 1
    th, tE = (torch.from_numpy(x).requires_grad_(True) for x in (h, E))
    loss = torch.nn.functional.cross_entropy(th @ tE.T, torch.from_numpy(a))
    (g * loss).backward()
    rloss, rows, dh, dE = R.ce_head(h, E, a, g)
    assert abs(rloss - loss.item()) <= 1e-12
    assert rows.shape == (B,) and abs(rows.mean() - rloss) <= 1e-15
    if V == 1:
        assert rloss == 0.0 and not rows.any() and not dh.any() and not dE.any()
        assert not th.grad.numpy().any() and not tE.grad.numpy().any()
        return
    assert rel_l2(dh, th.grad.numpy()) <= 1e-10
    assert rel_l2(dE, tE.grad.numpy()) <= 1e-10


def test_symbols_are_exported_and_bound():
    from bsarec_amd import _lib
    lib = _lib.load()
    for name in ("bsarec_ce_head_workspace_bytes", "bsarec_ce_head_fwd", "bsarec_ce_head_bwd"):
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes == _lib.EXPORTS[name][1]
    assert lib.bsarec_abi_version() == 10


BAD_SHAPES = [dict(B=0), dict(B=-1), dict(B=65537), dict(V=0), dict(V=-1), dict(d=0), dict(d=2), dict(d=66), dict(d=260)]


def test_workspace_bytes():
    from bsarec_amd import _lib
    f = _lib.load().bsarec_ce_head_workspace_bytes
    for B, V, d in ((1, 1, 4), (33, 1000, 100), (256, 3417, 64), (4096, 10_000_001, 256)):
        assert 0 < f(B, V, d) <= (16384 + 2 * B) * (d + 8) * 4, (B, V, d)
    assert f(256, 10 ** 6, 64) == f(256, 10 ** 7, 64)          # nothing in it grows with V
    for c in BAD_SHAPES:
        kw = dict(B=8, V=100, d=64)
        kw.update(c)
        assert f(kw["B"], kw["V"], kw["d"]) < 0, c


FWD = ["h", "ldh", "item_emb", "B", "V", "d", "answers", "loss_out", "rows_out", "workspace", "workspace_bytes", "stream"]
BWD = ["h", "ldh", "item_emb", "B", "V", "d", "answers", "gout", "workspace", "workspace_bytes", "dh", "d_item_emb", "stream"]
ENTRY = {"bsarec_ce_head_fwd": FWD, "bsarec_ce_head_bwd": BWD}
COMMON = BAD_SHAPES + [dict(ldh=60), dict(ldh=66), dict(h=None), dict(item_emb=None), dict(answers=None), dict(workspace=None),
                       dict(h="p+4"), dict(item_emb="p+4"), dict(workspace="p+4"), dict(workspace_bytes=0),
                       dict(workspace_bytes="short")]
CASES = ([(n, c) for n in ENTRY for c in COMMON] + [("bsarec_ce_head_fwd", dict(loss_out=None))] +
         [("bsarec_ce_head_bwd", c) for c in (dict(gout=None), dict(dh=None), dict(d_item_emb=None), dict(dh="p+4"),
                                              dict(d_item_emb="p+4"))])


@pytest.mark.parametrize("name,change", CASES, ids=[f"{n[15:]}-{'-'.join(f'{k}={v}' for k, v in c.items())}" for n, c in CASES])
def test_invalid_arguments_return_negative_without_a_gpu(name, change):
    from bsarec_amd import _lib
    lib = _lib.load()
    buf = (C.c_byte * 4096)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16           # a 16-byte aligned host address (never dereferenced)
    need = lib.bsarec_ce_head_workspace_bytes(8, 100, 64)
    kw = dict(h=p, ldh=3200, item_emb=p, B=8, V=100, d=64, answers=p, loss_out=p, rows_out=None, gout=p, workspace=p,
              workspace_bytes=need, dh=p, d_item_emb=p, stream=None)
    for k, v in change.items():
        kw[k] = {"p+4": p + 4, "short": need - 1}.get(v, v) if isinstance(v, str) else v
    assert getattr(lib, name)(*[kw[k] for k in ENTRY[name]]) < 0


def test_duorec_ce_head_flag_and_model_option():
    from bsarec_amd.main import parse_args
    assert not hasattr(parse_args([]), "duorec_ce_head")      # absent unless given: the logged arguments stay as they were
    assert parse_args(["--duorec_ce_head", "hip"]).duorec_ce_head == "hip"
    assert parse_args(["--duorec_ce_head", "torch"]).duorec_ce_head == "torch"
    with pytest.raises(SystemExit):
        parse_args(["--duorec_ce_head", "triton"])
    assert _model().duorec_ce_head == "torch"                 # the default namespace: torch.matmul + F.cross_entropy
    m = _model(duorec_ce_head="hip")
    assert m.duorec_ce_head == "hip" and m.duorec_head == "torch"      # independent of the contrastive head's flag
    with pytest.raises(ValueError, match="duorec_ce_head"):
        _model(duorec_ce_head="triton")
