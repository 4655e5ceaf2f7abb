"""The fused Mamba4Rec step on the host, no GPU: the fp64 restatement (mamba4rec_step_ref) against torch autograd and
torch.optim.Adam in double on a twin whose state-space layer is mamba_ref.torch_layer, the new symbols and their bindings, the
header as plain C, the weight count against ``mamba4rec_param_shapes``, every argument limit of the two entry points (they return
< 0 before any HIP call), the command-line flag and the model's mode switch with its flat weight array."""
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
import mamba_ref as M
import mamba4rec_step_ref as S

# V, d, N, L, B; expand, d_state, d_conv, dt_rank
SHAPES = [((11, 4, 1, 1, 3), (1, 4, 2, 4)), ((23, 12, 2, 7, 5), (2, 8, 4, 4)), ((17, 8, 1, 20, 4), (2, 16, 3, 4))]


def _params(rng, V, d, N, hyper):
    p = {"item_embeddings.weight": rng.normal(0, 0.5, (V, d))}
    for k in S.keys(N, hyper, d)[1:]:
        leaf = k.split(".")[-1]
        if ".mamba." in k and "LayerNorm" not in k:
            continue
        if "LayerNorm" in k:
            p[k] = (1.0 if leaf == "weight" else 0.0) + 0.1 * rng.normal(size=d)
        elif "dense_1" in k:
            p[k] = rng.normal(0, 1 / math.sqrt(d), (4 * d, d)) if leaf == "weight" else 0.1 * rng.normal(size=4 * d)
        else:
            p[k] = rng.normal(0, 1 / math.sqrt(4 * d), (d, 4 * d)) if leaf == "weight" else 0.1 * rng.normal(size=d)
    for k in range(N):
        flat = M.random_weights(rng, d, *hyper, std=0.3).astype(np.float64)
        for n, v in M.split_weights(flat, d, *hyper).items():
            p[f"item_encoder.blocks.{k}.mamba.{n}"] = v.copy()
    return {k: p[k] for k in S.keys(N, hyper, d)}


def _ln(x, w, b):
    xc = x - x.mean(-1, keepdim=True)
    return w * (xc / torch.sqrt((xc * xc).mean(-1, keepdim=True) + 1e-12)) + b


def _twin_loss(tp, ids, answers, N, hyper, mults):
    """Mamba4RecModel._encode / calculate_loss in torch double, the dropout multipliers given."""
    E = tp["item_embeddings.weight"]
    d = E.shape[1]
    x = _ln(E[ids], tp["LayerNorm.weight"], tp["LayerNorm.bias"]) * mults[0]
    for k in range(N):
        p = f"item_encoder.blocks.{k}."
        z = M.torch_layer(x, ids, {n: tp[p + "mamba." + n] for n in M.weight_shapes(d, *hyper)}, hyper)
        a = _ln(z * mults[1 + 2 * k] + x, tp[p + "mamba.LayerNorm.weight"], tp[p + "mamba.LayerNorm.bias"])
        f = a @ tp[p + "feed_forward.dense_1.weight"].T + tp[p + "feed_forward.dense_1.bias"]
        f = f * 0.5 * (1.0 + torch.erf(f / math.sqrt(2.0)))
        f = f @ tp[p + "feed_forward.dense_2.weight"].T + tp[p + "feed_forward.dense_2.bias"]
        x = _ln(f * mults[2 + 2 * k] + a, tp[p + "feed_forward.LayerNorm.weight"], tp[p + "feed_forward.LayerNorm.bias"])
    return torch.nn.functional.cross_entropy(x[:, -1] @ E.T, answers)


@pytest.mark.parametrize("wd", [0.0, 0.01])
@pytest.mark.parametrize("shape,hyper", SHAPES, ids=lambda s: "-".join(str(v) for v in s))
def test_reference_equals_autograd_and_torch_adam_in_double(shape, hyper, wd):
    V, d, N, L, B = shape
    rng = np.random.default_rng(V)
    params = _params(rng, V, d, N, hyper)
    first = list(rng.integers(0, L, B))
    first[0], first[1] = 0, L                                  # a full row, and a row of padding alone
    if B > 2:
        first[2] = L - 1                                       # a row whose first item is the last position
    ids = M.ragged_ids(rng, B, L, first, V)
    ans = rng.integers(1, V, B)
    ans[0] = ids[0, -1]                                        # a row that the lookup and the head both touch
    assert not ids[1].any() and ids[0].all() and ids[2, :L - 1].sum() == 0 and ids[2, L - 1] != 0
    tp = {k: torch.from_numpy(v.copy()).requires_grad_(True) for k, v in params.items()}
    # eps = 1e-3 in both optimisers: d(update) / d(g) is at most lr / eps, so the two gradients' last-bit differences (~1e-16)
    # stay far below the bound; at eps = 1e-8 a gradient element that happens to be near 0 multiplies them by up to 1e6
    opt = torch.optim.Adam(list(tp.values()), lr=1e-2, eps=1e-3, weight_decay=wd)
    st = S.adam_state(lr=1e-2, eps=1e-3, weight_decay=wd)
    tids, tans = torch.from_numpy(ids), torch.from_numpy(ans)
    for step in range(1, 4):
        mults = [(rng.random((B, L, d)) >= 0.5) * 2.0 for _ in range(1 + 2 * N)]       # explicit keep masks, p = 0.5
        rloss, rgrads, _ = S.loss_and_grads(params, ids, ans, N, hyper, mults)
        assert list(rgrads) == list(params) == S.keys(N, hyper, d)
        opt.zero_grad()
        loss = _twin_loss(tp, tids, tans, N, hyper, [torch.from_numpy(m) for m in mults])
        loss.backward()
        assert abs(rloss - loss.item()) <= 1e-12
        for k, p in tp.items():
            assert rgrads[k].shape == p.shape and np.abs(rgrads[k] - p.grad.numpy()).max() <= 1e-12, (step, k)
        opt.step()
        assert S.train_step(params, st, ids, ans, N, hyper, mults) == rloss
        for k, p in tp.items():
            assert np.abs(params[k] - p.detach().numpy()).max() <= 1e-12, (step, k)
    assert st.t == 3


NAMES = ("bsarec_mamba4rec_weight_floats", "bsarec_mamba4rec_workspace_bytes", "bsarec_mamba4rec_loss_grad",
         "bsarec_mamba4rec_train_step")


def test_symbols_are_exported_and_bound():
    from bsarec_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes == _lib.EXPORTS[name][1]
        assert getattr(lib, name).restype == _lib.EXPORTS[name][0]
    assert len(_lib.EXPORTS["bsarec_mamba4rec_loss_grad"][1]) == 13 and len(_lib.EXPORTS["bsarec_mamba4rec_train_step"][1]) == 10
    assert _lib.EXPORTS["bsarec_mamba4rec_loss_grad"][1][1:] == _lib.EXPORTS["bsarec_lrurec_loss_grad"][1][1:]
    assert _lib.EXPORTS["bsarec_mamba4rec_train_step"][1][1:] == _lib.EXPORTS["bsarec_lrurec_train_step"][1][1:]
    assert [f for f, _ in _lib.Mamba4RecConfig._fields_] == ["mamba", "layers", "item_size", "dropout", "ln_eps"]
    assert C.sizeof(_lib.Mamba4RecConfig) == C.sizeof(_lib.MambaConfig) + 16
    assert lib.bsarec_abi_version() == 10 and _lib.ABI_VERSION == 10          # additive: the version stays


def test_header_block_is_plain_c99_and_links(tmp_path):
    lib_dir = os.path.join(ROOT, "bsarec_amd")
    if not os.path.exists(os.path.join(lib_dir, "libbsarec_hip.so")) or not shutil.which("gcc"):
        pytest.skip("library or gcc missing")
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
    f = tmp_path / "host.c"
    f.write_text(src)
    exe = tmp_path / "host"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(f), "-o", str(exe),
                    "-L", lib_dir, "-lbsarec_hip", f"-Wl,-rpath,{lib_dir}"], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    ver, ws, lws, nw, m, bad = (int(v) for v in r.stdout.split())
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
ADAM_PTRS = ["params", "grads", "exp_avg", "exp_avg_sq"]
CASES = [(n, c) for n in ENTRY for c in BAD_CFG] + [(n, dict(cfg=None)) for n in ENTRY]
CASES += [(n, {p: v}) for n in ENTRY for p in PTRS16[n] + PTRS8 for v in (None, "p+4")]
CASES += [(n, dict(loss_out=v)) for n in ENTRY for v in (None, "p+2")]
CASES += [(n, dict(workspace_bytes=v)) for n in ENTRY for v in (0, "short")]
T = "bsarec_mamba4rec_train_step"
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
    return _lib.Mamba4RecConfig(_lib.MambaConfig(c["batch"], c["seq_len"], c["width"], c["expand"], c["d_state"], c["d_conv"],
                                                 c["dt_rank"]), c["layers"], c["item_size"], c["dropout"], c["ln_eps"])


def _id(n, c):
    return f"{n[16:]}-" + "-".join(f"{k}={v}" for k, v in c.items())


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


def _call(name, change):
    from bsarec_amd import _lib
    lib = _lib.load()
    buf = (C.c_byte * 4096)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16           # a 16-byte aligned host address (never dereferenced)
    need = lib.bsarec_mamba4rec_workspace_bytes(_cfg())
    n = {"adam_items": GOOD["item_size"] * GOOD["width"], "adam_weights": lib.bsarec_mamba4rec_weight_floats(_cfg())}
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
    assert not hasattr(parse_args([]), "mamba_step")               # absent unless given: the logged arguments stay as they were
    assert parse_args(["--model_type", "Mamba4Rec", "--mamba_step", "fused"]).mamba_step == "fused"
    assert parse_args(["--mamba_step", "torch"]).mamba_step == "torch"
    with pytest.raises(SystemExit):
        parse_args(["--mamba_step", "graph"])


def test_mode_switch_and_the_flat_array_on_the_host():
    from bsarec_amd import Mamba4RecModel
    from bsarec_amd.mamba4rec import mamba4rec_param_shapes
    hyper = (2, 16, 4, 4)                                          # the layer's defaults at d = 8
    assert Mamba4RecModel.torch_optim is True and Mamba4RecModel.own_train_step is False
    torch.manual_seed(3)
    default = Mamba4RecModel(_args())
    torch.manual_seed(3)
    fused = Mamba4RecModel(_args(mamba_step="fused"))
    torch_mode = Mamba4RecModel(_args(mamba_step="torch"))
    assert default.mamba_step == torch_mode.mamba_step == "torch" and default.torch_optim is True
    assert torch_mode.torch_optim is True and default.own_train_step is False and default._wflat is None
    assert fused.mamba_step == "fused" and fused.torch_optim is False and fused.own_train_step is True
    assert fused.needs_negatives is False
    with pytest.raises(ValueError, match="mamba_step must be 'torch' or 'fused'"):
        Mamba4RecModel(_args(mamba_step="bogus"))
    # the same keys, shapes and (same seed) values in both modes; checkpoints pass between them
    sd, sf = default.state_dict(), fused.state_dict()
    assert list(sd) == list(sf) == S.keys(2, hyper, 8)
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
        for (k, shp), q in zip(mamba4rec_param_shapes(8, 2, *hyper).items(), m.flat_parameters()):
            if q.data_ptr() != flat.data_ptr() + 4 * off or tuple(q.shape) != shp or q is not dict(m.named_parameters())[k]:
                return False
            off += q.numel()
        for k, blk in enumerate(m.item_encoder.blocks):         # each layer's array is a slice of it, and the layer agrees
            la = blk.mamba
            o = m._wslices[f"item_encoder.blocks.{k}.mamba.in_proj.weight"][0]
            if la._flat.data_ptr() != flat.data_ptr() + 4 * o or la._flat.numel() != M.weight_floats(8, *hyper):
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
    with pytest.raises(RuntimeError, match="mamba_step = 'fused'"):
        default.loss_and_grads(ids, ids[:, 0])
    with pytest.raises(RuntimeError, match="MI355X"):               # no CPU path for the fused step either
        fused.train_step(ids, ids[:, 0])
    with pytest.raises(RuntimeError, match="MI355X"):
        fused.loss_and_grads(ids, ids[:, 0])
