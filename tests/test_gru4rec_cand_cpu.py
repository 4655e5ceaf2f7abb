"""The GRU4Rec heads over shared candidates on the host, no GPU: the fp64 restatement (gru4rec_cand_ref) against torch autograd in
double on the formulas of the contract, the batch whose rows have no negative, the new symbols and their bindings, the header as
plain C, every argument limit of the entry points (they return < 0 before any HIP call), the command-line flags and the
combinations of loss and negatives that the model refuses."""
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
import gru4rec_cand_ref as R

B, V, D = 17, 5, 8
COMBOS = [(l, n) for l in R.LOSSES for n in R.NEGATIVES]


def _inputs():
    g = torch.Generator().manual_seed(21)
    s = torch.randn(B, D, generator=g, dtype=torch.float64)
    E = torch.randn(V, D, generator=g, dtype=torch.float64) * 0.7
    pos = torch.randint(0, V, (B,), generator=g)
    neg = torch.randint(0, V, (B,), generator=g)
    neg[3] = pos[3]                                           # a negative equal to its own row's answer
    return s, E, pos, neg


def _autograd_loss(s, E, pos, neg, loss, negatives, bpreg):
    """The contract, row by row, in torch ops."""
    cand = pos if negatives == "in_batch" else torch.cat([pos, neg])
    r = s @ E[cand].T
    rows = []
    for b in range(s.shape[0]):
        j = torch.nonzero(cand != pos[b]).reshape(-1)
        if j.numel() == 0:
            rows.append(r[b, b] * 0.0)
            continue
        x, xb = r[b, j], r[b, b]
        if loss == "ce":
            rows.append(torch.logsumexp(torch.cat([xb.reshape(1), x]), 0) - xb)
        elif loss == "top1":
            rows.append((torch.sigmoid(x - xb) + torch.sigmoid(x * x)).mean())
        else:
            p = torch.softmax(x, 0)
            rows.append(-torch.log((p * torch.sigmoid(xb - x)).sum() + 1e-10) + bpreg * (p * x * x).sum())
    return torch.stack(rows).mean(), r


@pytest.mark.parametrize("loss,negatives", COMBOS)
def test_reference_equals_autograd_in_double(loss, negatives):
    from bsarec_amd.gru4rec import cand_head_loss
    s, E, pos, neg = _inputs()
    bpreg = 0.7
    mask = R.negative_mask(pos.numpy(), neg.numpy(), negatives)
    assert mask.sum(1).min() > 0 and (~mask).sum(1).max() > 1          # V = 5: every row has negatives and masked columns
    rl, G, ds, dEc = R.head(s.numpy(), E.numpy(), pos.numpy(), neg.numpy(), loss, negatives, bpreg)
    st, Et = s.clone().requires_grad_(True), E.clone().requires_grad_(True)
    val, r = _autograd_loss(st, Et, pos, neg, loss, negatives, bpreg)
    r.retain_grad()
    val.backward()
    dE = np.zeros((V, D))
    np.add.at(dE, R.candidates(pos.numpy(), neg.numpy(), negatives), dEc)
    errs = (abs(rl - val.item()), np.abs(G - r.grad.numpy()).max(), np.abs(ds - st.grad.numpy()).max(),
            np.abs(dE - Et.grad.numpy()).max())
    print(f"cand ref {loss} {negatives}: loss {rl:.12f} errors {errs}")
    assert max(errs) <= 1e-12
    # the model's torch-op head (gru_step = "torch") is the same function
    s2, E2 = s.clone().requires_grad_(True), E.clone().requires_grad_(True)
    v2 = cand_head_loss(s2, E2, pos, neg, loss, negatives, bpreg)
    v2.backward()
    assert abs(v2.item() - rl) <= 1e-12
    assert np.abs(s2.grad.numpy() - ds).max() <= 1e-12 and np.abs(E2.grad.numpy() - dE).max() <= 1e-12


@pytest.mark.parametrize("loss", R.LOSSES)
def test_all_answers_equal_in_batch_is_exactly_zero(loss):
    from bsarec_amd.gru4rec import cand_head_loss
    s, E, pos, neg = _inputs()
    pos = torch.full_like(pos, 3)
    rl, G, ds, dEc = R.head(s.numpy(), E.numpy(), pos.numpy(), neg.numpy(), loss, "in_batch")
    assert rl == 0.0 and not G.any() and not ds.any() and not dEc.any()
    s2, E2 = s.clone().requires_grad_(True), E.clone().requires_grad_(True)
    v = cand_head_loss(s2, E2, pos, neg, loss, "in_batch")
    v.backward()
    assert v.item() == 0.0 and not s2.grad.any() and not E2.grad.any()
    # with the negatives behind them the rows have columns again
    assert R.head(s.numpy(), E.numpy(), pos.numpy(), neg.numpy(), loss, "in_batch+sampled")[0] > 0.0


NAMES = ("bsarec_gru4rec_cand_head_workspace_bytes", "bsarec_gru4rec_cand_head", "bsarec_gru4rec_cand_workspace_bytes",
         "bsarec_gru4rec_cand_loss_grad", "bsarec_gru4rec_cand_train_step")


def test_symbols_are_exported_and_bound():
    from bsarec_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes == _lib.EXPORTS[name][1]
        assert getattr(lib, name).restype == _lib.EXPORTS[name][0]
    assert len(_lib.EXPORTS["bsarec_gru4rec_cand_loss_grad"][1]) == 15
    assert len(_lib.EXPORTS["bsarec_gru4rec_cand_train_step"][1]) == 12
    assert len(_lib.EXPORTS["bsarec_gru4rec_cand_head"][1]) == 14
    assert [f for f, _ in _lib.Gru4RecHead._fields_] == ["loss", "candidates", "bpreg"] and C.sizeof(_lib.Gru4RecHead) == 12
    assert _lib.GRU4REC_LOSSES == {"ce": 1, "top1": 2, "bpr_max": 3}
    assert _lib.GRU4REC_CANDIDATES == {"in_batch": 1, "in_batch+sampled": 2}
    assert lib.bsarec_abi_version() == _lib.ABI_VERSION          # additions only: the version of the parent


def test_header_block_is_plain_c99_and_links(tmp_path):
    lib_dir = os.path.join(ROOT, "bsarec_amd")
    if not os.path.exists(os.path.join(lib_dir, "libbsarec_hip.so")) or not shutil.which("gcc"):
        pytest.skip("library or gcc missing")
    src = r"""
#include "bsarec_hip.h"
#include <stdio.h>
int main(void) {
    bsarec_gru4rec_config_t cfg = {{256, 50, 64, 64, 2, 64}, 3417, 0.5f};
    bsarec_gru4rec_head_t head = {3, 2, 1.0f};
    long base = bsarec_gru4rec_workspace_bytes(&cfg), ws = bsarec_gru4rec_cand_workspace_bytes(&cfg, &head);
    long alone = bsarec_gru4rec_cand_head_workspace_bytes(256, 64, &head), bad;
    int (*hd)(const float *, const float *, const int64_t *, const int64_t *, int, int, int, const bsarec_gru4rec_head_t *,
              float *, float *, float *, void *, long, void *) = bsarec_gru4rec_cand_head;
    int (*lg)(const bsarec_gru4rec_config_t *, const float *, const float *, const int64_t *, const int64_t *, const int64_t *,
              void *, int, float *, float *, float *, void *, long, void *, const bsarec_gru4rec_head_t *)
        = bsarec_gru4rec_cand_loss_grad;
    int (*ts)(const bsarec_gru4rec_config_t *, const int64_t *, const int64_t *, const int64_t *, const bsarec_adam_t *,
              const bsarec_adam_t *, void *, float *, void *, long, void *, const bsarec_gru4rec_head_t *)
        = bsarec_gru4rec_cand_train_step;
    head.loss = 4;
    bad = bsarec_gru4rec_cand_workspace_bytes(&cfg, &head);
    printf("%d %ld %ld %ld %ld\n", BSAREC_GRU4REC_CAND_MAX, base, ws, alone, bad);
    return (hd && lg && ts && ws > base && alone > 0 && bad < 0) ? 0 : 1;
}
"""
    f = tmp_path / "host.c"
    f.write_text(src)
    exe = tmp_path / "host"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(f), "-o", str(exe),
                    "-L", lib_dir, "-lbsarec_hip", f"-Wl,-rpath,{lib_dir}"], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    cmax, base, ws, alone, bad = (int(v) for v in r.stdout.split())
    # the documented layout at B = 256, C = 512, d = 64: nslab = min(16, 512 / 64) = 8
    Bq, Cq, d, ns = 256, 512, 64, 8
    head = Bq * Cq + ns * Cq * d + ns * Bq * d
    assert cmax == 8192 and ws == base + 4 * (head + Cq * d) and alone == 4 * (head + Bq)


GOOD = dict(batch=8, seq_len=10, input_size=64, hidden_size=64, num_layers=2, out_size=64, item_size=50, dropout=0.5)
GOOD_HEAD = dict(loss=1, candidates=2, bpreg=1.0)
BAD_HEAD = [dict(loss=0), dict(loss=4), dict(loss=-1), dict(candidates=0), dict(candidates=3), dict(bpreg=-0.5),
            dict(bpreg=float("nan")), dict(batch=8193, candidates=1), dict(batch=4097, candidates=2)]
BAD_CFG = [dict(batch=0), dict(batch=65537), dict(seq_len=0), dict(seq_len=257), dict(input_size=66, out_size=66),
           dict(input_size=260, out_size=260), dict(hidden_size=48), dict(num_layers=0), dict(num_layers=5),
           dict(out_size=32), dict(out_size=0), dict(input_size=32), dict(item_size=1), dict(item_size=0), dict(item_size=-7),
           dict(dropout=-0.1), dict(dropout=1.0), dict(dropout=1.5), dict(dropout=float("nan"))]
LOSS_GRAD = ["cfg", "item_emb", "weights", "ids", "answers", "neg_answers", "state", "train", "loss_out", "d_item_emb", "dweights",
             "workspace", "workspace_bytes", "stream", "head"]
TRAIN_STEP = ["cfg", "ids", "answers", "neg_answers", "adam_items", "adam_weights", "state", "loss_out", "workspace",
              "workspace_bytes", "stream", "head"]
HEAD = ["s", "item_emb", "answers", "neg_answers", "batch", "input_size", "item_size", "head", "loss_out", "ds", "dEc", "workspace",
        "workspace_bytes", "stream"]
LG, TS, HD = "bsarec_gru4rec_cand_loss_grad", "bsarec_gru4rec_cand_train_step", "bsarec_gru4rec_cand_head"
ENTRY = {LG: LOSS_GRAD, TS: TRAIN_STEP, HD: HEAD}
PTRS16 = {LG: ["item_emb", "weights", "d_item_emb", "dweights", "workspace"], TS: ["workspace"],
          HD: ["s", "item_emb", "ds", "dEc", "workspace"]}
PTRS8 = {LG: ["ids", "answers", "neg_answers", "state"], TS: ["ids", "answers", "neg_answers", "state"],
         HD: ["answers", "neg_answers"]}
ADAM_PTRS = ["params", "grads", "exp_avg", "exp_avg_sq"]
CASES = [(n, c) for n in ENTRY for c in BAD_HEAD] + [(n, dict(head=None)) for n in ENTRY]
CASES += [(n, c) for n in (LG, TS) for c in BAD_CFG] + [(n, dict(cfg=None)) for n in (LG, TS)]
CASES += [(HD, c) for c in (dict(batch=0), dict(batch=65537), dict(input_size=66), dict(input_size=260), dict(input_size=0),
                            dict(item_size=1), dict(item_size=-7))]
CASES += [(n, {p: v}) for n in ENTRY for p in PTRS16[n] + PTRS8[n] for v in (None, "p+4")]
CASES += [(n, dict(loss_out=v)) for n in ENTRY for v in (None, "p+2")]
CASES += [(n, dict(workspace_bytes=v)) for n in ENTRY for v in (0, "short")]
CASES += [(n, dict(workspace_bytes="pairwise")) for n in (LG, TS)]         # the pairwise step's size is too small
CASES += [(TS, {a: None}) for a in ("adam_items", "adam_weights")]
CASES += [(TS, {f"{a}.{p}": v}) for a in ("adam_items", "adam_weights") for p in ADAM_PTRS for v in (None, "p+4")]
CASES += [(TS, {f"{a}.n": v}) for a in ("adam_items", "adam_weights") for v in ("n+4", "n-4", 0)]
CASES += [(TS, {f"{a}.{k}": v}) for a in ("adam_items", "adam_weights")
          for k, v in (("shadow_bf16", "p"), ("grads2", "p"), ("grads2_n", 4), ("n_grad_srcs", 1), ("wimage_plan", "p"))]
CASES += [(TS, {"adam_weights.lr": 2e-3}), (TS, {"adam_weights.beta1": 0.8}), (TS, {"adam_items.beta2": 0.99})]


def _cfg(**kw):
    from bsarec_amd import _lib
    c = dict(GOOD)
    c.update({k: v for k, v in kw.items() if k in GOOD})
    gru = _lib.GruConfig(*[c[k] for k in ("batch", "seq_len", "input_size", "hidden_size", "num_layers", "out_size")])
    return _lib.Gru4RecConfig(gru, c["item_size"], c["dropout"])


def _head(**kw):
    from bsarec_amd import _lib
    h = dict(GOOD_HEAD)
    h.update({k: v for k, v in kw.items() if k in GOOD_HEAD})
    return _lib.Gru4RecHead(h["loss"], h["candidates"], h["bpreg"])


def _id(n, c):
    return f"{n[15:]}-" + "-".join(f"{k}={v}" for k, v in c.items())


def test_workspace_queries():
    from bsarec_amd import _lib
    lib = _lib.load()
    base = lib.bsarec_gru4rec_workspace_bytes(_cfg())
    one, two = (lib.bsarec_gru4rec_cand_workspace_bytes(_cfg(), _head(candidates=c)) for c in (1, 2))
    assert two > one > base > 0
    assert lib.bsarec_gru4rec_cand_workspace_bytes(_cfg(), _head(loss=3, bpreg=0.0)) == two
    assert lib.bsarec_gru4rec_cand_workspace_bytes(_cfg(batch=8192), _head(candidates=1)) > 0          # C = 8192 is inside
    assert lib.bsarec_gru4rec_cand_workspace_bytes(_cfg(batch=4096), _head(candidates=2)) > 0
    assert lib.bsarec_gru4rec_cand_head_workspace_bytes(8192, 256, _head(candidates=1)) > 0
    assert lib.bsarec_gru4rec_cand_workspace_bytes(None, _head()) < 0
    assert lib.bsarec_gru4rec_cand_workspace_bytes(_cfg(), None) < 0
    assert lib.bsarec_gru4rec_cand_head_workspace_bytes(8, 64, None) < 0
    for change in BAD_CFG:
        assert lib.bsarec_gru4rec_cand_workspace_bytes(_cfg(**change), _head()) < 0, change
    for change in BAD_HEAD:
        assert lib.bsarec_gru4rec_cand_workspace_bytes(_cfg(**change), _head(**change)) < 0, change
        assert lib.bsarec_gru4rec_cand_head_workspace_bytes(change.get("batch", 8), 64, _head(**change)) < 0, change
    for batch, width in ((0, 64), (65537, 64), (8, 66), (8, 260), (8, 0)):
        assert lib.bsarec_gru4rec_cand_head_workspace_bytes(batch, width, _head()) < 0, (batch, width)


@pytest.mark.parametrize("name,change", CASES, ids=[_id(n, c) for n, c in CASES])
def test_invalid_arguments_return_negative_without_a_gpu(name, change):
    from bsarec_amd import _lib
    lib = _lib.load()
    buf = (C.c_byte * 4096)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16           # a 16-byte aligned host address (never dereferenced)
    alone = name == HD
    cfg_change = {k: v for k, v in change.items() if k in GOOD}
    cfg, head = _cfg(**cfg_change), _head(**change)
    # the good shape's size; a case that changes the shape gets a size no shape needs
    need = (lib.bsarec_gru4rec_cand_head_workspace_bytes(GOOD["batch"], GOOD["input_size"], _head()) if alone
            else lib.bsarec_gru4rec_cand_workspace_bytes(_cfg(), _head()))
    assert need > 0
    n = {"adam_items": GOOD["item_size"] * GOOD["input_size"], "adam_weights": lib.bsarec_gru_weight_floats(_cfg().gru)}
    adam = {a: _lib.Adam(p, p, p, p, n[a], 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, None, 0) for a in n}
    kw = dict(cfg=cfg, head=head, s=p, item_emb=p, weights=p, ids=p, answers=p, neg_answers=p, state=p, train=1, loss_out=p,
              d_item_emb=p, dweights=p, ds=p, dEc=p, workspace=p, workspace_bytes=1 << 40, stream=None,
              batch=GOOD["batch"], input_size=GOOD["input_size"], item_size=GOOD["item_size"], **adam)
    if not cfg_change and "workspace_bytes" not in change:
        kw["workspace_bytes"] = need
    for k, v in change.items():
        if k in GOOD_HEAD:
            continue
        if k in GOOD:
            kw[k] = v
        elif "." in k:
            a, field = k.split(".")
            v = {"p": p, "p+4": p + 4, "n+4": n[a] + 4, "n-4": n[a] - 4}.get(v, v) if isinstance(v, str) else v
            if field == "n_grad_srcs":
                adam[a].grad_srcs[0] = p
            setattr(adam[a], field, v)
        else:
            pairwise = lib.bsarec_gru4rec_workspace_bytes(_cfg())
            kw[k] = {"p+4": p + 4, "p+2": p + 2, "short": need - 1, "pairwise": pairwise}.get(v, v) if isinstance(v, str) else v
    assert getattr(lib, name)(*[kw[k] for k in ENTRY[name]]) < 0


def test_the_limit_cases_start_inside_the_limits():
    """The shape the cases above perturb is inside the limits: the queries answer, and the pairwise step's size is smaller than
    the candidate step's (so the "pairwise" case tests the size, nothing else)."""
    from bsarec_amd import _lib
    lib = _lib.load()
    assert 0 < lib.bsarec_gru4rec_workspace_bytes(_cfg()) < lib.bsarec_gru4rec_cand_workspace_bytes(_cfg(), _head())
    assert lib.bsarec_gru4rec_cand_head_workspace_bytes(GOOD["batch"], GOOD["input_size"], _head()) > 0


def _args(**kw):
    a = argparse.Namespace(item_size=301, hidden_size=64, gru_hidden_size=64, num_hidden_layers=2, max_seq_length=20,
                           hidden_dropout_prob=0.5, initializer_range=0.02)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_command_line_flags():
    from bsarec_amd.main import parse_args
    a = parse_args([])
    assert not any(hasattr(a, k) for k in ("gru_loss", "gru_negatives", "gru_bpreg"))      # absent unless given
    a = parse_args(["--model_type", "GRU4Rec", "--gru_step", "fused", "--gru_loss", "bpr_max", "--gru_negatives",
                    "in_batch+sampled", "--gru_bpreg", "0.5"])
    assert (a.gru_loss, a.gru_negatives, a.gru_bpreg) == ("bpr_max", "in_batch+sampled", 0.5)
    for loss in ("bpr", "ce", "top1", "bpr_max"):
        assert parse_args(["--gru_loss", loss]).gru_loss == loss
    for bad in (["--gru_loss", "softmax"], ["--gru_negatives", "sampled"], ["--gru_bpreg", "much"]):
        with pytest.raises(SystemExit):
            parse_args(bad)


def test_flag_combinations():
    from bsarec_amd import GRU4RecModel
    default = GRU4RecModel(_args())
    assert (default.gru_loss, default.gru_negatives, default._head) == ("bpr", "pair", None)
    assert GRU4RecModel(_args(gru_loss="bpr", gru_negatives="pair"))._head is None
    for loss, code in (("ce", 1), ("top1", 2), ("bpr_max", 3)):
        for negatives, cand in (("in_batch", 1), ("in_batch+sampled", 2)):
            for step in ("torch", "fused"):
                m = GRU4RecModel(_args(gru_loss=loss, gru_negatives=negatives, gru_step=step, gru_bpreg=0.25))
                assert (m._head.loss, m._head.candidates, m._head.bpreg) == (code, cand, 0.25)
                assert m.torch_optim is (step == "torch")
                assert list(m.state_dict()) == list(default.state_dict())
    assert GRU4RecModel(_args(gru_loss="bpr_max", gru_negatives="in_batch"))._head.bpreg == 1.0
    for loss, negatives in (("bpr", "in_batch"), ("bpr", "in_batch+sampled"), ("ce", "pair"), ("top1", "pair"),
                            ("bpr_max", "pair"), ("ce", None), (None, "in_batch")):
        kw = {k: v for k, v in (("gru_loss", loss), ("gru_negatives", negatives)) if v is not None}
        with pytest.raises(ValueError, match="gru_loss.*gru_negatives"):
            GRU4RecModel(_args(**kw))
    with pytest.raises(ValueError, match="gru_loss"):
        GRU4RecModel(_args(gru_loss="softmax", gru_negatives="in_batch"))
    with pytest.raises(ValueError, match="gru_negatives"):
        GRU4RecModel(_args(gru_loss="ce", gru_negatives="sampled"))
    for bad in (-1.0, math.nan):
        with pytest.raises(ValueError, match="gru_bpreg"):
            GRU4RecModel(_args(gru_loss="bpr_max", gru_negatives="in_batch", gru_bpreg=bad))
    ids = torch.randint(1, 301, (3, 20))
    fused = GRU4RecModel(_args(gru_loss="ce", gru_negatives="in_batch", gru_step="fused"))
    with pytest.raises(RuntimeError, match="MI355X"):               # no CPU path for the candidate step either
        fused.train_step(ids, ids[:, 0], ids[:, 1])
