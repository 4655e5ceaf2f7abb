"""FEARec without a GPU: the fp64 restatement (fearec_ref) against a literal torch.fft restatement, the identities the kernels
rest on, its backward against autograd, the band table, the C entries' limits, the flags, the registration and the refusals."""
import argparse
import math
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import fearec_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("bsarec_fea_attn_workspace_bytes", "bsarec_fea_attn_fwd", "bsarec_fea_attn_bwd")
CASES = [((3, 6, 8), 3, 4, 2), ((3, 7, 12), 0, 4, 2), ((4, 12, 8), 2, 7, 2), ((2, 50, 16), 10, 26, 3), ((2, 2, 4), 0, 2, 1)]


@pytest.mark.parametrize("shape,lo,hi,k", CASES)
@pytest.mark.parametrize("train", [True, False])
def test_reference_equals_the_literal_fft_restatement(shape, lo, hi, k, train):
    Q, K, V = R.random_case(shape, 11)
    out, m, idx, p = R.forward(Q, K, V, lo, hi, k, train)
    tq, tk, tv = (torch.from_numpy(a).double() for a in (Q, K, V))
    rows = np.broadcast_to(idx, (shape[0], k))
    tied = bool(R.ambiguous(m.mean(0) if train else m, k, 1e-9).any())     # the Nyquist bin alone: m = c (-1)^tau, exact ties
    assert tied == ((lo, hi) == (3, 4))
    tout, tm, tidx = R.torch_attention(tq, tk, tv, lo, hi, k, train, idx=rows if tied else None)
    assert np.abs(m - tm.numpy()).max() <= 1e-13 * max(1.0, np.abs(m).max())
    assert (np.sort(rows, 1) == np.sort(tidx.numpy(), 1)).all()
    if tied:                                                                # ... which the rule gives to the lower delays
        assert not R.ambiguous(m.mean(0) if train else m, k, 1e-9, exact_ties=True).any()
        assert (np.diff(rows, axis=1) == 2).all() and (rows[:, 0] < 2).all()
    assert np.abs(out - tout.numpy()).max() <= 1e-12
    # the same with torch.roll, as the layer is usually written
    ref = sum(p[:, i, None, None] * np.stack([np.roll(V[b].astype(np.float64), -rows[b, i], axis=0) for b in range(shape[0])])
              for i in range(k))
    assert np.abs(out - ref).max() <= 1e-12


def test_full_band_is_the_circular_cross_correlation_and_the_time_domain_form_holds():
    for L in (6, 7, 50):
        Q, K, _ = R.random_case((2, L, 8), L)
        F = L // 2 + 1
        m = R.mean_corr(Q, K, 0, F)
        q, k = Q.astype(np.float64), K.astype(np.float64)
        cc = np.stack([(np.roll(q, -tau, axis=1) * k).sum((1, 2)) for tau in range(L)], 1) / 8
        assert np.abs(m - cc).max() <= 2e-14 * np.abs(cc).max() * L
        # what the kernels compute: the Gram matrix's diagonal sums r against the band's impulse response h
        for lo, hi in ((0, 1), (1, 3), (F - 1, F), (0, F)):
            f = np.arange(lo, hi)[:, None]
            w = np.where((f == 0) | (2 * f == L), 1.0, 2.0)
            h = (w * np.cos(2 * np.pi * ((f * np.arange(L)[None]) % L) / L)).sum(0) / L
            r = np.stack([(q * np.roll(k, -dl, axis=1)).sum((1, 2)) for dl in range(L)], 1)
            mt = np.stack([(r * h[(np.arange(L) + tau) % L]).sum(1) for tau in range(L)], 1) / 8
            assert np.abs(mt - R.mean_corr(Q, K, lo, hi)).max() <= 1e-13 * np.abs(r).max()


@pytest.mark.parametrize("shape,lo,hi,k", CASES)
@pytest.mark.parametrize("train", [True, False])
def test_backward_equals_autograd_in_double(shape, lo, hi, k, train):
    Q, K, V = R.random_case(shape, 5)
    dOut = np.random.default_rng(6).standard_normal(shape)
    _, _, idx, _ = R.forward(Q, K, V, lo, hi, k, train)
    dQ, dK, dV = R.backward(Q, K, V, dOut, lo, hi, idx)
    tq, tk, tv = (torch.from_numpy(a).double().requires_grad_(True) for a in (Q, K, V))
    tout, _, _ = R.torch_attention(tq, tk, tv, lo, hi, k, train, idx=np.broadcast_to(idx, (shape[0], k)))
    (tout * torch.from_numpy(dOut)).sum().backward()
    # (absolute beside relative: with the Nyquist bin alone both chosen delays have one parity, and dQ = dK = 0 identically)
    for got, ref in ((dQ, tq.grad), (dK, tk.grad), (dV, tv.grad)):
        assert np.abs(got - ref.numpy()).max() <= 1e-13 * max(1.0, float(ref.abs().max()))
    if (lo, hi) == (3, 4):
        assert np.abs(dQ).max() <= 1e-15 and np.abs(dK).max() <= 1e-15
        aQ, aK, _ = R.backward(Q, K, V, dOut, lo, hi, idx, absolute=True)
        assert np.abs(aQ).max() > 1e-3 and np.abs(aK).max() > 1e-3


def test_band_table_and_topk():
    from bsarec_amd.fearec import fea_bands, fea_topk
    table = {(50, 2, 0.6): [(10, 26), (0, 16)], (50, 2, 0.3): [(13, 26), (0, 13)],
             (50, 4, 0.6): [(10, 26), (7, 23), (4, 20), (1, 17)], (12, 2, 0.6): [(2, 7), (0, 5)]}
    for (L, N, g), want in table.items():
        assert fea_bands(L, N, g) == want == R.bands(L, N, g)
    assert fea_bands(50, 1, 0.6) == [(0, 26)]
    for bad in ((50, 2, 0.0), (50, 2, 1.5), (50, 0, 0.6), (2, 8, 0.1)):
        with pytest.raises(ValueError):
            fea_bands(*bad)
    assert fea_topk(50) == 3 == R.topk(50) and fea_topk(2) == 1 and fea_topk(12, 1.0) == 2
    assert fea_topk(256, 100.0) == 32 and fea_topk(8, 100.0) == 8 and fea_topk(50, 0.01) == 1


def test_symbols_are_exported_and_bound():
    from bsarec_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes == _lib.EXPORTS[name][1]
        assert getattr(lib, name).restype == _lib.EXPORTS[name][0]
    assert [f[0] for f in _lib.FeaAttnConfig._fields_] == ["batch", "seq_len", "width", "lo", "hi", "topk", "train"]
    assert lib.bsarec_abi_version() == 10 and _lib.ABI_VERSION == 10
    cfg = lambda *a: _lib.FeaAttnConfig(*a)
    # m [B, L] | idx | p | h | cv, in 4-byte words, each part rounded up to 4
    assert lib.bsarec_fea_attn_workspace_bytes(cfg(5, 50, 64, 10, 26, 3, 1)) == 4 * (252 + 4 + 16 + 52 + 252)
    assert lib.bsarec_fea_attn_workspace_bytes(cfg(5, 50, 64, 10, 26, 3, 0)) == 4 * (252 + 16 + 16 + 52 + 252)
    assert lib.bsarec_fea_attn_workspace_bytes(cfg(65536, 256, 256, 0, 129, 32, 0)) > 0
    assert lib.bsarec_fea_attn_workspace_bytes(cfg(1, 2, 4, 0, 2, 1, 1)) > 0
    for bad in ((0, 50, 64, 10, 26, 3, 1), (65537, 50, 64, 10, 26, 3, 1), (5, 1, 64, 0, 1, 1, 1), (5, 257, 64, 0, 16, 3, 1),
                (5, 50, 0, 10, 26, 3, 1), (5, 50, 6, 10, 26, 3, 1), (5, 50, 260, 10, 26, 3, 1), (5, 50, 64, -1, 26, 3, 1),
                (5, 50, 64, 10, 10, 3, 1), (5, 50, 64, 12, 10, 3, 1), (5, 50, 64, 10, 27, 3, 1), (5, 7, 64, 0, 5, 3, 1),
                (5, 50, 64, 10, 26, 0, 1), (5, 50, 64, 10, 26, 33, 1), (5, 6, 64, 0, 4, 7, 1)):
        assert lib.bsarec_fea_attn_workspace_bytes(cfg(*bad)) < 0, bad
    assert lib.bsarec_fea_attn_workspace_bytes(None) < 0


LIMITS_C = r"""
#include "bsarec_hip.h"
#include <stdio.h>
static long long buf[4096];                                       /* never dereferenced by a refused call */
#define P4 ((const float *)((char *)buf + 4))
#define P16 ((float *)(((unsigned long)buf + 64) & ~15ul))
static int bad = 0, cases = 0;
static void neg(int rc, int line) { ++cases; if (rc >= 0) { printf("line %d returned %d\n", line, rc); ++bad; } }
#define NEG(call) neg((int)(call), __LINE__)
#define REFUSED(call) neg((int)(call) == -10 ? -10 : 0, __LINE__)   /* the code itself: BSAREC's invalid-argument return */
#define FWD(c, q, k, v, o, ws, wsb) bsarec_fea_attn_fwd(c, q, k, v, o, ws, wsb, 0)
#define BWD(c, q, k, v, g, ws, wsb, dq, dk, dv) bsarec_fea_attn_bwd(c, q, k, v, g, ws, wsb, dq, dk, dv, 0)
int main(void) {
    bsarec_fea_attn_config_t ok = {5, 50, 64, 10, 26, 3, 1}, c;
    long w = bsarec_fea_attn_workspace_bytes(&ok);
    if (w <= 0) { printf("workspace %ld\n", w); return 2; }
    /* shapes: each limit on both sides, through the query and through both entries */
#define SHAPE(field, value) c = ok; c.field = value; NEG(bsarec_fea_attn_workspace_bytes(&c)); \
    NEG(FWD(&c, P16, P16, P16, P16, P16, w)); NEG(BWD(&c, P16, P16, P16, P16, P16, w, P16, P16, P16));
    SHAPE(batch, 0) SHAPE(batch, 65537) SHAPE(seq_len, 1) SHAPE(seq_len, 257) SHAPE(width, 0) SHAPE(width, 6) SHAPE(width, 260)
    SHAPE(lo, -1) SHAPE(lo, 26) SHAPE(hi, 10) SHAPE(hi, 27) SHAPE(topk, 0) SHAPE(topk, 33)
    c = ok; c.seq_len = 6; c.lo = 0; c.hi = 4; c.topk = 7; NEG(bsarec_fea_attn_workspace_bytes(&c));   /* topk > L */
    c = ok; c.seq_len = 7; c.lo = 0; c.hi = 5; NEG(bsarec_fea_attn_workspace_bytes(&c));               /* odd L: F = 4 */
    NEG(bsarec_fea_attn_workspace_bytes(0));
    /* pointers: null, then misaligned; the workspace size */
    NEG(FWD(0, P16, P16, P16, P16, P16, w));
    NEG(FWD(&ok, 0, P16, P16, P16, P16, w));    NEG(FWD(&ok, P16, 0, P16, P16, P16, w));    NEG(FWD(&ok, P16, P16, 0, P16, P16, w));
    NEG(FWD(&ok, P16, P16, P16, 0, P16, w));    NEG(FWD(&ok, P16, P16, P16, P16, 0, w));
    NEG(FWD(&ok, P4, P16, P16, P16, P16, w));   NEG(FWD(&ok, P16, P4, P16, P16, P16, w));   NEG(FWD(&ok, P16, P16, P4, P16, P16, w));
    NEG(FWD(&ok, P16, P16, P16, (float *)P4, P16, w));   NEG(FWD(&ok, P16, P16, P16, P16, (void *)P4, w));
    NEG(FWD(&ok, P16, P16, P16, P16, P16, w - 1));       NEG(FWD(&ok, P16, P16, P16, P16, P16, 0));
    NEG(BWD(0, P16, P16, P16, P16, P16, w, P16, P16, P16));
    NEG(BWD(&ok, 0, P16, P16, P16, P16, w, P16, P16, P16));     NEG(BWD(&ok, P16, 0, P16, P16, P16, w, P16, P16, P16));
    NEG(BWD(&ok, P16, P16, 0, P16, P16, w, P16, P16, P16));     NEG(BWD(&ok, P16, P16, P16, 0, P16, w, P16, P16, P16));
    NEG(BWD(&ok, P16, P16, P16, P16, 0, w, P16, P16, P16));     NEG(BWD(&ok, P16, P16, P16, P16, P16, w, 0, P16, P16));
    NEG(BWD(&ok, P16, P16, P16, P16, P16, w, P16, 0, P16));     NEG(BWD(&ok, P16, P16, P16, P16, P16, w, P16, P16, 0));
    NEG(BWD(&ok, P16, P16, P16, P4, P16, w, P16, P16, P16));    NEG(BWD(&ok, P16, P16, P16, P16, P16, w, (float *)P4, P16, P16));
    NEG(BWD(&ok, P16, P16, P16, P16, P16, w, P16, (float *)P4, P16));
    NEG(BWD(&ok, P16, P16, P16, P16, P16, w, P16, P16, (float *)P4));
    NEG(BWD(&ok, P16, P16, P16, P16, P16, w - 1, P16, P16, P16));
    REFUSED(BWD(&ok, P4, P16, P16, P16, P16, w, P16, P16, P16));    REFUSED(BWD(&ok, P16, P4, P16, P16, P16, w, P16, P16, P16));
    REFUSED(BWD(&ok, P16, P16, P4, P16, P16, w, P16, P16, P16));    REFUSED(BWD(&ok, P16, P16, P16, P16, (void *)P4, w, P16, P16, P16));
    printf("%d cases, %d bad, abi %d\n", cases, bad, bsarec_abi_version());
    return bad ? 1 : 0;
}
"""


def test_header_is_plain_c_and_every_limit_returns_negative_without_a_gpu(tmp_path):
    lib_dir = os.path.join(ROOT, "bsarec_amd")
    if not os.path.exists(os.path.join(lib_dir, "libbsarec_hip.so")) or not shutil.which("gcc"):
        pytest.skip("library or gcc missing")
    f = tmp_path / "limits.c"
    f.write_text(LIMITS_C)
    exe = tmp_path / "limits"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(f), "-o", str(exe),
                    "-L", lib_dir, "-lbsarec_hip", f"-Wl,-rpath,{lib_dir}"], check=True, capture_output=True)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")          # no device: a HIP call could not succeed
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 bad, abi 10"), r.stdout
    assert int(r.stdout.split()[0]) == 13 * 3 + 3 + 13 + 18                          # every NEG line above ran


def _ns(**kw):
    base = dict(item_size=50, hidden_size=16, max_seq_length=12, batch_size=4, hidden_dropout_prob=0.1,
                attention_probs_dropout_prob=0.1, num_hidden_layers=2, num_attention_heads=2, hidden_act="gelu",
                initializer_range=0.02, seed=1)
    base.update(kw)
    return argparse.Namespace(**base)


def test_flags_are_absent_unless_given_and_reject_bad_values():
    from bsarec_amd import main as M
    a = M.parse_args([])
    for name in ("global_ratio", "spatial_ratio", "fredom", "fredom_type", "fea_topk_factor"):
        assert not hasattr(a, name)
    a = M.parse_args(["--model_type", "FEARec", "--global_ratio", "0.4", "--spatial_ratio", "0", "--fredom", "False",
                      "--fredom_type", "su", "--fea_topk_factor", "2.5"])
    assert (a.global_ratio, a.spatial_ratio, a.fredom, a.fredom_type, a.fea_topk_factor) == (0.4, 0.0, False, "su", 2.5)
    assert M.parse_args(["--fredom", "True", "--global_ratio", "1", "--spatial_ratio", "1"]).fredom is True
    for flag, bads in (("--global_ratio", ("0", "1.5", "-0.2", "nan", "x")), ("--spatial_ratio", ("-0.1", "1.01", "nan", "x")),
                       ("--fredom", ("true", "1", "yes")), ("--fredom_type", ("us", "x")),
                       ("--fea_topk_factor", ("0", "-1", "nan", "inf", "x"))):
        for bad in bads:
            with pytest.raises(SystemExit):
                M.parse_args([flag, bad])


def test_registration_leaves_the_pinned_tables_alone():
    import bsarec_amd
    from bsarec_amd import FEARecModel, FeaAttention, main as M, model as Mo
    from bsarec_amd.fearec import FEARecModel as F2
    assert FEARecModel is F2 and "fearec" in M.MODEL_REGISTRY and M.MODEL_REGISTRY["fearec"] is FEARecModel
    assert M.model_class("FEARec") is FEARecModel and M.model_class("fearec") is FEARecModel
    assert "FEARecModel" in bsarec_amd.__all__ and "FeaAttention" in bsarec_amd.__all__ and FeaAttention is not None
    assert set(Mo.MODEL_DICT) == {"bsarec", "sasrec", "fmlprec", "duorec", "gru4rec"}
    assert set(M.MODEL_DICT) == set(Mo.MODEL_DICT) | {"caser"}
    assert M.SIBLING_MODELS == {"bert4rec": bsarec_amd.BERT4RecModel}
    assert M.model_class("bsarec") is Mo.BSARecModel and M.model_class("BERT4Rec") is bsarec_amd.BERT4RecModel
    with pytest.raises(KeyError):
        M.model_class("fearec2")


def test_state_dict_is_sasrecs_and_loads_both_ways():
    from bsarec_amd import FEARecModel, SASRecModel
    torch.manual_seed(3)
    fea, sas = FEARecModel(_ns()), SASRecModel(_ns())
    fsd, ssd = fea.state_dict(), sas.state_dict()
    assert len(fsd) == 36 and list(fsd) == list(ssd)
    assert {k: tuple(v.shape) for k, v in fsd.items()} == {k: tuple(v.shape) for k, v in ssd.items()}
    for k, v in fsd.items():                                       # SASRec's init: N(0, range) weights, zero biases, LN (1, 0)
        if "LayerNorm.weight" in k:
            assert (v == 1).all()
        elif k.endswith(".bias"):
            assert (v == 0).all()
        else:
            assert 0.5 * 0.02 < float(v.std()) < 1.5 * 0.02
    fea.load_state_dict(ssd)
    for k, v in fea.state_dict().items():
        assert torch.equal(v.cpu(), ssd[k].cpu()), k
    fea2 = FEARecModel(_ns())
    sas.load_state_dict(fea2.state_dict())
    for k, v in sas.state_dict().items():
        assert torch.equal(v.cpu(), fea2.state_dict()[k].cpu()), k
    assert fea.bands == [(2, 7), (0, 5)] and fea.topk == 2
    assert [b.layer.fea.lo for b in fea.item_encoder.blocks] == [2, 0]


def test_interface_and_refusals():
    from bsarec_amd import FEARecModel, FeaAttention
    args = _ns()
    m = FEARecModel(args)
    assert m.needs_negatives is False and m.needs_same_target is True and m.torch_optim is True and m.full_logits is None
    assert m.catalogue_weight().shape == (50, 16) and not m.catalogue_weight().requires_grad
    assert (m.global_ratio, m.spatial_ratio, m.fredom, m.fredom_type) == (0.6, 0.1, True, "us_x")
    for kw, msg in ((dict(storage="bf16"), "bf16"), (dict(train_negatives=8), "train_negatives"),
                    (dict(train_lazy_adam=True), "train_lazy_adam"), (dict(global_ratio=0.0), "global_ratio"),
                    (dict(global_ratio=1.5), "global_ratio"), (dict(spatial_ratio=-0.1), "spatial_ratio"),
                    (dict(spatial_ratio=float("nan")), "spatial_ratio"), (dict(fredom_type="us"), "fredom_type"),
                    (dict(fea_topk_factor=0.0), "fea_topk_factor"), (dict(duorec_head="x"), "duorec_head"),
                    (dict(duorec_ce_head="x"), "duorec_ce_head"), (dict(max_seq_length=1), "max_seq_length"),
                    (dict(max_seq_length=300), "max_seq_length"), (dict(hidden_size=18, num_attention_heads=1), "hidden_size"),
                    (dict(num_hidden_layers=8, max_seq_length=2, global_ratio=0.1), "band")):
        with pytest.raises(ValueError, match=msg):
            FEARecModel(_ns(**kw))
    with pytest.raises(ValueError, match="FEARec: single GPU only"):
        m.check_trainer(args, object())
    m.check_trainer(args, None)
    for step in (m.train_step, m.grad_step):
        with pytest.raises(RuntimeError, match="FEARec steps through"):
            step(None, None)
    ids = torch.ones(4, 12, dtype=torch.int64)
    for call in (lambda: m.calculate_loss(ids, torch.ones(4, dtype=torch.int64), None, ids), lambda: m(ids),
                 lambda: m.last_hidden(ids), lambda: m.predict(ids)):
        with pytest.raises(RuntimeError, match="MI355X"):
            call()
    attn = FeaAttention(12, 16, 2, 7, 2)
    x = torch.zeros(4, 12, 16)
    with pytest.raises(RuntimeError, match="MI355X"):
        attn(x, x, x)
    with pytest.raises(RuntimeError, match="MI355X"):
        attn(x.requires_grad_(True), x, x)
    for bad in ((1, 16, 0, 1, 1), (12, 18, 2, 7, 2), (12, 16, 7, 7, 2), (12, 16, 2, 8, 2), (12, 16, 2, 7, 0), (12, 16, 2, 7, 13)):
        with pytest.raises(ValueError):
            FeaAttention(*bad)


def test_spectral_distance_is_the_ortho_rfft_modulus():
    from bsarec_amd import FEARecModel
    m = FEARecModel(_ns()).double()
    g = torch.Generator().manual_seed(0)
    a, b = torch.randn(3, 12, 16, generator=g, dtype=torch.float64), torch.randn(3, 12, 16, generator=g, dtype=torch.float64)
    want = R.Twin.spectral_distance(a, b)
    assert abs(float(m.spectral_distance(a, b)) - float(want)) <= 1e-14
    a.requires_grad_(True)
    m.spectral_distance(a, a.detach().clone()).backward()           # |0|: the modulus passes 0, not NaN
    assert torch.isfinite(a.grad).all() and float(a.grad.abs().max()) == 0.0
    assert math.isclose(float(m.spectral_distance(a.detach(), a.detach())), 0.0)
