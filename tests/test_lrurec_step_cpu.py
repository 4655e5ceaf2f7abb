"""The fused LRURec step on the host, no GPU: the fp64 restatement (lrurec_step_ref) against torch autograd and torch.optim.Adam in
double on a twin whose recurrent layer runs on torch complex tensors, the new symbols and their bindings, the header as plain C,
the weight count against ``lrurec_param_shapes``, every argument limit of the two entry points (they return < 0 before any HIP
call), the command-line flag and the model's mode switch with its flat weight array."""
import argparse
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import ROOT
import lru_ref as R
import lrurec_step_ref as S

SHAPES = [(11, 4, 1, 1, 3), (23, 12, 2, 7, 5), (17, 8, 1, 20, 4)]          # V, d, N, L, B


def _params(rng, V, d, N):
    p = {"item_embeddings.weight": rng.normal(0, 0.5, (V, d))}
    for k in S.keys(N, d)[1:]:
        leaf = k.split(".")[-1]
        if ".lru." in k and "LayerNorm" not in k:
            continue
        if "LayerNorm" in k:
            p[k] = (1.0 if leaf == "weight" else 0.0) + 0.1 * rng.normal(size=d)
        elif "dense_1" in k:
            p[k] = rng.normal(0, 1 / math.sqrt(d), (4 * d, d)) if leaf == "weight" else 0.1 * rng.normal(size=4 * d)
        else:
            p[k] = rng.normal(0, 1 / math.sqrt(4 * d), (d, 4 * d)) if leaf == "weight" else 0.1 * rng.normal(size=d)
    for k in range(N):
        for n, v in R.split_weights(R.random_weights(rng, d).astype(np.float64), d).items():
            p[f"item_encoder.blocks.{k}.lru.{n}"] = v.copy()
    return {k: p[k] for k in S.keys(N, d)}


def _ln(x, w, b):
    xc = x - x.mean(-1, keepdim=True)
    return w * (xc / torch.sqrt((xc * xc).mean(-1, keepdim=True) + 1e-12)) + b


def _twin_loss(tp, ids, answers, N, mults):
    """LRURecModel._encode / calculate_loss in torch double, the dropout multipliers given."""
    E = tp["item_embeddings.weight"]
    d = E.shape[1]
    x = _ln(E[ids], tp["LayerNorm.weight"], tp["LayerNorm.bias"]) * mults[0]
    for k in range(N):
        p = f"item_encoder.blocks.{k}."
        z = R.torch_complex_layer(x, ids, {n: tp[p + "lru." + n] for n in R.weight_shapes(d)})
        a = _ln(z * mults[1 + 2 * k] + x, tp[p + "lru.LayerNorm.weight"], tp[p + "lru.LayerNorm.bias"])
        f = a @ tp[p + "feed_forward.dense_1.weight"].T + tp[p + "feed_forward.dense_1.bias"]
        f = f * 0.5 * (1.0 + torch.erf(f / math.sqrt(2.0)))
        f = f @ tp[p + "feed_forward.dense_2.weight"].T + tp[p + "feed_forward.dense_2.bias"]
        x = _ln(f * mults[2 + 2 * k] + a, tp[p + "feed_forward.LayerNorm.weight"], tp[p + "feed_forward.LayerNorm.bias"])
    return torch.nn.functional.cross_entropy(x[:, -1] @ E.T, answers)


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "V%d-d%d-N%d-L%d-B%d" % s)
def test_reference_equals_autograd_and_torch_adam_in_double(shape, wd):
    V, d, N, L, B = shape
    rng = np.random.default_rng(V)
    params = _params(rng, V, d, N)
    first = list(rng.integers(0, L, B))
    first[0], first[1] = 0, L                                  # a full row, and a row of padding alone
    if B > 2:
        first[2] = L - 1                                       # a row whose first item is the last position
    ids = R.ragged_ids(rng, B, L, first, V)
    ans = rng.integers(1, V, B)
    ans[0] = ids[0, -1]                                        # a row that the lookup and the head both touch
    assert not ids[1].any() and ids[0].all()
    tp = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in params.items()}
    # eps = 1e-3 in both optimisers: d(update) / d(g) is at most lr / eps, so the two gradients' last-bit differences (~1e-16)
    # stay far below the bound; at eps = 1e-8 a gradient element that happens to be near 0 multiplies them by up to 1e6
    opt = torch.optim.Adam(list(tp.values()), lr=1e-2, eps=1e-3, weight_decay=wd)
    st = S.adam_state(lr=1e-2, eps=1e-3, weight_decay=wd)
    tids, tans = torch.from_numpy(ids), torch.from_numpy(ans)
    for step in range(1, 4):
        mults = [(rng.random((B, L, d)) >= 0.5) * 2.0 for _ in range(1 + 2 * N)]       # explicit keep masks, p = 0.5
        rloss, rgrads, _ = S.loss_and_grads(params, ids, ans, N, mults)
        assert list(rgrads) == list(params) == S.keys(N, d)
        opt.zero_grad()
        loss = _twin_loss(tp, tids, tans, N, [torch.from_numpy(m) for m in mults])
        loss.backward()
        assert abs(rloss - loss.item()) <= 1e-12
        for k, p in tp.items():
            assert rgrads[k].shape == p.shape and np.abs(rgrads[k] - p.grad.numpy()).max() <= 1e-12, (step, k)
        opt.step()
        assert S.train_step(params, st, ids, ans, N, mults) == rloss
        for k, p in tp.items():
            assert np.abs(params[k] - p.detach().numpy()).max() <= 1e-12, (step, k)
    assert st.t == 3


def test_philox_multipliers():
    m = S.dropout_mults(3, 5, 8, 2, 0.5, 1234567, 2)
    assert len(m) == 5 and all(set(np.unique(a)) == {0.0, 2.0} and a.shape == (3, 5, 8) for a in m)
    assert not np.array_equal(m[0], m[1])
    assert all(np.array_equal(a, np.ones((3, 5, 8))) for a in S.dropout_mults(3, 5, 8, 2, 0.0, 1, 1))


NAMES = ("bsarec_lrurec_weight_floats", "bsarec_lrurec_workspace_bytes", "bsarec_lrurec_loss_grad", "bsarec_lrurec_train_step")


def test_symbols_are_exported_and_bound():
    from bsarec_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes == _lib.EXPORTS[name][1]
        assert getattr(lib, name).restype == _lib.EXPORTS[name][0]
    assert len(_lib.EXPORTS["bsarec_lrurec_loss_grad"][1]) == 13 and len(_lib.EXPORTS["bsarec_lrurec_train_step"][1]) == 10
    assert [f for f, _ in _lib.LruRecConfig._fields_] == ["lru", "layers", "item_size", "dropout", "ln_eps"]
    assert C.sizeof(_lib.LruRecConfig) == C.sizeof(_lib.LruConfig) + 16
    assert lib.bsarec_abi_version() == 10 and _lib.ABI_VERSION == 10          # additive: the version stays


def test_header_block_is_plain_c99_and_links(tmp_path):
    lib_dir = os.path.join(ROOT, "bsarec_amd")
    if not os.path.exists(os.path.join(lib_dir, "libbsarec_hip.so")) or not shutil.which("gcc"):
        pytest.skip("library or gcc missing")
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
    f = tmp_path / "host.c"
    f.write_text(src)
    exe = tmp_path / "host"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(f), "-o", str(exe),
                    "-L", lib_dir, "-lbsarec_hip", f"-Wl,-rpath,{lib_dir}"], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ver, ws, lws, nw, bad = (int(v) for v in r.stdout.split())
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
ADAM_PTRS = ["params", "grads", "exp_avg", "exp_avg_sq"]
CASES = [(n, c) for n in ENTRY for c in BAD_CFG] + [(n, dict(cfg=None)) for n in ENTRY]
CASES += [(n, {p: v}) for n in ENTRY for p in PTRS16[n] + PTRS8 for v in (None, "p+4")]
CASES += [(n, dict(loss_out=v)) for n in ENTRY for v in (None, "p+2")]
CASES += [(n, dict(workspace_bytes=v)) for n in ENTRY for v in (0, "short")]
T = "bsarec_lrurec_train_step"
CASES += [(T, {a: None}) for a in ("adam_items", "adam_weights")]
CASES += [(T, {f"{a}.{p}": v}) for a in ("adam_items", "adam_weights") for p in ADAM_PTRS for v in (None, "p+4")]
CASES += [(T, {f"{a}.n": v}) for a in ("adam_items", "adam_weights") for v in ("n+4", "n-4", 0)]
CASES += [(T, {f"{a}.{k}": v}) for a in ("adam_items", "adam_weights")
          for k, v in (("shadow_bf16", "p"), ("grads2", "p"), ("grads2_n", 4), ("n_grad_srcs", 1), ("wimage_plan", "p"))]
CASES += [(T, {"adam_weights.lr": 2e-3}), (T, {"adam_weights.beta1": 0.8}), (T, {"adam_items.beta2": 0.99})]


def _cfg(**kw):
    from bsarec_amd import _lib
    c = dict(GOOD)
    c.update(kw)
    return _lib.LruRecConfig(_lib.LruConfig(c["batch"], c["seq_len"], c["width"]), c["layers"], c["item_size"], c["dropout"],
                             c["ln_eps"])


def _id(n, c):
    return f"{n[14:]}-" + "-".join(f"{k}={v}" for k, v in c.items())


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


def _call(name, change):
    from bsarec_amd import _lib
    lib = _lib.load()
    buf = (C.c_byte * 4096)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16           # a 16-byte aligned host address (never dereferenced)
    need = lib.bsarec_lrurec_workspace_bytes(_cfg())
    n = {"adam_items": GOOD["item_size"] * GOOD["width"], "adam_weights": lib.bsarec_lrurec_weight_floats(_cfg())}
    adam = {a: _lib.Adam(p, p, p, p, n[a], 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, None, 0) for a in n}
    kw = dict(cfg=_cfg(), item_emb=p, weights=p, ids=p, answers=p, state=p, train=1, loss_out=p, d_item_emb=p, dweights=p,
              workspace=p, workspace_bytes=need, stream=None, **adam)
    for k, v in change.items():
        if k in GOOD:
            kw["cfg"] = _cfg(**change)
        elif "." in k:
            a, field = k.split(".")
            v = {"p": p, "p+4": p + 4, "n+4": n[a] + 4, "n-4": n[a] - 4}.get(v, v) if isinstance(v, str) else v
            if field == "n_grad_srcs":
                adam[a].grad_srcs[0] = p
            setattr(adam[a], field, v)
        else:
            kw[k] = {"p+4": p + 4, "p+2": p + 2, "short": need - 1}.get(v, v) if isinstance(v, str) else v
    return getattr(lib, name)(*[kw[k] for k in ENTRY[name]])


@pytest.mark.parametrize("name,change", CASES, ids=[_id(n, c) for n, c in CASES])
def test_invalid_arguments_return_negative_without_a_gpu(name, change):
    assert _call(name, change) < 0


def _args(**kw):
    a = argparse.Namespace(item_size=41, hidden_size=8, num_hidden_layers=2, max_seq_length=6, hidden_dropout_prob=0.5,
                           initializer_range=0.02)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_command_line_flag():
    from bsarec_amd.main import parse_args
    assert not hasattr(parse_args([]), "lru_step")                 # absent unless given: the logged arguments stay as they were
    assert parse_args(["--model_type", "LRURec", "--lru_step", "fused"]).lru_step == "fused"
    assert parse_args(["--lru_step", "torch"]).lru_step == "torch"
    with pytest.raises(SystemExit):
        parse_args(["--lru_step", "graph"])


def test_mode_switch_and_the_flat_array_on_the_host():
    from bsarec_amd import LRURecModel
    from bsarec_amd.lrurec import lrurec_param_shapes
    assert LRURecModel.torch_optim is True and LRURecModel.own_train_step is False
    torch.manual_seed(3)
    default = LRURecModel(_args())
    torch.manual_seed(3)
    fused = LRURecModel(_args(lru_step="fused"))
    torch_mode = LRURecModel(_args(lru_step="torch"))
    assert default.lru_step == torch_mode.lru_step == "torch" and default.torch_optim is True and torch_mode.torch_optim is True
    assert default.own_train_step is False and default._wflat is None
    assert fused.lru_step == "fused" and fused.torch_optim is False and fused.own_train_step is True
    assert fused.needs_negatives is False
    with pytest.raises(ValueError, match="lru_step"):
        LRURecModel(_args(lru_step="bogus"))
    # the same keys, shapes and (same seed) values in both modes; checkpoints pass between them
    sd, sf = default.state_dict(), fused.state_dict()
    assert list(sd) == list(sf) == S.keys(2, 8)
    for k in sd:
        assert sd[k].shape == sf[k].shape and torch.equal(sd[k], sf[k]), k
    with torch.no_grad():
        for q in fused.parameters():
            q.add_(0.25)
    torch_mode.load_state_dict(fused.state_dict())
    default.load_state_dict(torch_mode.state_dict())
    fused.load_state_dict(default.state_dict())

    def is_flat(m):
        flat, off = m._wflat, 0
        for (k, shp), q in zip(lrurec_param_shapes(8, 2).items(), m.flat_parameters()):
            if q.data_ptr() != flat.data_ptr() + 4 * off or tuple(q.shape) != shp or q is not dict(m.named_parameters())[k]:
                return False
            off += q.numel()
        for k, blk in enumerate(m.item_encoder.blocks):         # each layer's array is a slice of it, and the layer agrees
            la = blk.lru
            o = m._wslices[f"item_encoder.blocks.{k}.lru.nu_log"][0]
            if la._flat.data_ptr() != flat.data_ptr() + 4 * o or la._flat.numel() != 4 * 8 * 8 + 6 * 8:
                return False
            held = la._flat
            la.reflatten()                                        # the pointer test accepts a slice: nothing is rebuilt
            if la._flat is not held:
                return False
        return off == flat.numel() and flat.data_ptr() % 16 == 0

    assert is_flat(fused)
    values = {k: v.clone() for k, v in fused.state_dict().items()}
    moved = fused.double().float()                                # gives every parameter a storage of its own, twice
    assert moved is fused and is_flat(fused)
    for k, v in fused.state_dict().items():
        assert torch.equal(v, values[k]), k
    ids = torch.randint(1, 41, (3, 6))
    with pytest.raises(RuntimeError, match="torch.optim.Adam"):
        default.train_step(ids, ids[:, 0])
    with pytest.raises(RuntimeError, match="lru_step = 'fused'"):
        default.loss_and_grads(ids, ids[:, 0])
    with pytest.raises(RuntimeError, match="MI355X"):               # no CPU path for the fused step either
        fused.train_step(ids, ids[:, 0])
    with pytest.raises(RuntimeError, match="MI355X"):
        fused.loss_and_grads(ids, ids[:, 0])
