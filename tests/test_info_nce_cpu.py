"""DuoRec's HIP contrastive head on the host, no GPU: the fp64 restatement (info_nce_ref) against autograd through
DuoRecModel.info_nce + F.cross_entropy, the exported symbols, the argument checks of the three entry points (they return
< 0 before any HIP call), and the --duorec_head flag."""
import argparse
import ctypes as C
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import GOLDEN, rel_l2
import info_nce_ref as R


def _model(**kw):
    from bsarec_amd import DuoRecModel
    z = np.load(os.path.join(GOLDEN, "duorec_A_d64_L50_h2.npz"))
    cfg = json.loads(str(z["cfg"]))
    return DuoRecModel(argparse.Namespace(hidden_act="gelu", batch_size=10, c=3, **cfg, **kw))


@pytest.fixture(scope="module")
def model():
    return _model()


def _inputs(B, d, sim, seed):
    rng = np.random.default_rng(seed)
    zi, zj = rng.normal(0, 1, (B, d)), rng.normal(0, 1, (B, d))
    if B >= 2:
        zj[1] = zi[0]                                        # a duplicated row (and not a positive pair)
    zero = None
    if sim == "cos" and B >= 2:
        zero = B                                             # one all-zero row, z_j[0]: never the duplicated row z_j[1]
        zj[0] = 0.0
    return zi, zj, zero


@pytest.mark.parametrize("sim", ["dot", "cos"])
@pytest.mark.parametrize("B", [1, 2, 5, 33])
@pytest.mark.parametrize("tau", [1.0, 0.2])
def test_reference_equals_autograd_through_the_torch_head(model, sim, B, tau):
    d, g = 12, 0.37
    zi, zj, zero = _inputs(B, d, sim, seed=B)
    ti, tj = (torch.from_numpy(a).requires_grad_(True) for a in (zi, zj))
    loss = torch.nn.functional.cross_entropy(*model.info_nce(ti, tj, tau, B, sim))
    (g * loss).backward()
    want = np.concatenate([ti.grad.numpy(), tj.grad.numpy()])
    rloss, rows, dzi, dzj = R.info_nce(zi, zj, tau, sim, g)
    got = np.concatenate([dzi, dzj])
    assert abs(rloss - loss.item()) <= 1e-12
    assert rows.shape == (2 * B,) and abs(rows.mean() - rloss) <= 1e-15
    if B == 1:
        assert rloss == 0.0 and not got.any() and not want.any()
        return
    rest = np.ones(2 * B, bool)
    if zero is not None:                                     # ~1e7 in magnitude: on its own relative scale
        rest[zero] = False
        assert np.linalg.norm(want[zero]) > 1e5
        assert rel_l2(got[zero], want[zero]) <= 1e-10
    assert rel_l2(got[rest], want[rest]) <= 1e-10


def test_symbols_are_exported_and_bound():
    from bsarec_amd import _lib
    lib = _lib.load()
    for name in ("bsarec_info_nce_workspace_bytes", "bsarec_info_nce_fwd", "bsarec_info_nce_bwd"):
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes == _lib.EXPORTS[name][1]
    assert lib.bsarec_abi_version() == 10


BAD_SHAPES = [dict(B=0), dict(B=-1), dict(B=4097), dict(d=0), dict(d=2), dict(d=66), dict(d=260), dict(sim=2), dict(sim=-1)]


def test_workspace_bytes():
    from bsarec_amd import _lib
    f = _lib.load().bsarec_info_nce_workspace_bytes
    for B, d in ((1, 4), (33, 100), (256, 64), (4096, 256)):
        for sim in (0, 1):
            assert f(B, d, sim) >= 4 * 4 * B                 # at least lse and the norms of 2B rows
    assert f(512, 64, 0) < 3 * f(256, 64, 0)                 # linear in B, not quadratic
    for c in BAD_SHAPES:
        kw = dict(B=8, d=64, sim=0)
        kw.update(c)
        assert f(kw["B"], kw["d"], kw["sim"]) < 0, c


FWD = ["z_i", "ld_i", "z_j", "ld_j", "B", "d", "inv_tau", "sim", "loss_out", "rows_out", "workspace", "workspace_bytes", "stream"]
BWD = ["z_i", "ld_i", "z_j", "ld_j", "B", "d", "inv_tau", "sim", "gout", "workspace", "workspace_bytes", "dz_i", "dz_j", "stream"]
ENTRY = {"bsarec_info_nce_fwd": FWD, "bsarec_info_nce_bwd": BWD}
COMMON = BAD_SHAPES + [dict(ld_i=60), dict(ld_j=60), dict(ld_i=66), dict(ld_j=3202), dict(z_i=None), dict(z_j=None),
                       dict(z_i="p+4"), dict(z_j="p+8"), dict(workspace=None), dict(workspace="p+4"), dict(workspace_bytes=0),
                       dict(workspace_bytes="short"), dict(inv_tau=0.0), dict(inv_tau=-1.0), dict(inv_tau=float("inf")),
                       dict(inv_tau=float("nan"))]
CASES = ([(n, c) for n in ENTRY for c in COMMON] + [("bsarec_info_nce_fwd", dict(loss_out=None))] +
         [("bsarec_info_nce_bwd", c) for c in (dict(gout=None), dict(dz_i=None), dict(dz_j=None), dict(dz_i="p+4"), dict(dz_j="p+4"))])


@pytest.mark.parametrize("name,change", CASES, ids=[f"{n[16:]}-{'-'.join(f'{k}={v}' for k, v in c.items())}" for n, c in CASES])
def test_invalid_arguments_return_negative_without_a_gpu(name, change):
    from bsarec_amd import _lib
    lib = _lib.load()
    buf = (C.c_byte * 4096)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16           # a 16-byte aligned host address (never dereferenced)
    need = lib.bsarec_info_nce_workspace_bytes(8, 64, 0)
    kw = dict(z_i=p, ld_i=64, z_j=p, ld_j=3200, B=8, d=64, inv_tau=5.0, sim=0, loss_out=p, rows_out=None, gout=p, workspace=p,
              workspace_bytes=need, dz_i=p, dz_j=p, stream=None)
    for k, v in change.items():
        kw[k] = {"p+4": p + 4, "p+8": p + 8, "short": need - 1}.get(v, v) if isinstance(v, str) else v
    assert getattr(lib, name)(*[kw[k] for k in ENTRY[name]]) < 0


def test_duorec_head_flag_and_model_option(model):
    from bsarec_amd.main import parse_args
    from bsarec_amd.model import DUOREC_HEADS
    assert DUOREC_HEADS == ("torch", "hip")
    assert not hasattr(parse_args([]), "duorec_head")         # absent unless given: the logged arguments stay as they were
    assert parse_args(["--duorec_head", "hip"]).duorec_head == "hip"
    assert parse_args(["--duorec_head", "torch"]).duorec_head == "torch"
    with pytest.raises(SystemExit):
        parse_args(["--duorec_head", "triton"])
    assert model.duorec_head == "torch"                       # the default namespace: the restated torch head
    assert _model(duorec_head="hip").duorec_head == "hip"
    with pytest.raises(ValueError, match="duorec_head"):
        _model(duorec_head="triton")
