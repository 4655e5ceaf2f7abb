"""BERT4Rec's pieces on the host, no GPU: the fp64 restatement (cloze_ref) against torch in double, the masking rules, the oracle
under the padding-only mask against finite differences, the new symbols and their bindings, the header as plain C, every
argument limit of the entry points (< 0 before any HIP call, through a stand-alone C program), the driver's flags and tables,
and the model's refusals."""
import argparse
import os
import shutil
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from conftest import ROOT  # noqa: E402
import cloze_ref as R  # noqa: E402


def test_reference_head_equals_torch_in_double():
    rng = np.random.default_rng(0)
    T, V, d, Rn, n = 40, 23, 8, 16, 11
    h, E = rng.normal(0, 1, (T, d)), rng.normal(0, 1, (V + 1, d))
    rows = np.full(Rn, -1, np.int32)
    rows[:n] = np.sort(rng.choice(T, n, replace=False))
    targets = np.zeros(Rn, np.int64)
    targets[:n] = rng.integers(0, V, n)
    loss, out_rows, dh, dE = R.cloze_head(h, E[:V], rows, targets, n, g=0.37)
    th, tE = torch.tensor(h, requires_grad=True), torch.tensor(E, requires_grad=True)
    idx, a = torch.from_numpy(rows[:n].astype(np.int64)), torch.from_numpy(targets[:n])
    tl = torch.nn.functional.cross_entropy(th[idx] @ tE[:V].T, a, reduction="sum") / n
    (0.37 * tl).backward()
    assert abs(loss - tl.item()) <= 1e-12
    assert np.abs(dh - th.grad.numpy()).max() <= 1e-12 and np.abs(dE - tE.grad.numpy()[:V]).max() <= 1e-12
    assert not tE.grad.numpy()[V].any() and not out_rows[n:].any()
    per_row = torch.nn.functional.cross_entropy(th[idx] @ tE[:V].T, a, reduction="none").detach().numpy()
    assert np.abs(out_rows[:n] - per_row).max() <= 1e-12
    zero = R.cloze_head(h, E[:V], rows, targets, 0)
    assert zero[0] == 0.0 and not zero[2].any() and not zero[3].any()


def _ids(B, L, V, seed):
    rng = np.random.default_rng(seed)
    ids = np.zeros((B, L), np.int64)
    for b in range(B):
        n = 0 if b == 0 else (L if b == 1 else int(rng.integers(1, L + 1)))
        if n:
            ids[b, L - n:] = rng.integers(1, V, size=n)
    return ids


def test_mask_rules():
    B, L, V = 7, 50, 99
    ids = _ids(B, L, V, 1)
    # ratio = 0: only the forced last position of every non-empty row
    masked, rows, targets, n = R.cloze_mask(ids, 0.0, 20, 5, 1, V)
    assert n == B - 1 and list(rows[:n]) == [b * L + L - 1 for b in range(1, B)]
    assert np.array_equal(targets[:n], ids[1:, L - 1]) and (masked == V).sum() == n
    assert (rows[n:] == -1).all() and not targets[n:].any()
    # an all-padding row gives nothing, whatever the ratio
    for ratio in (0.2, 1.0):
        masked, rows, targets, n = R.cloze_mask(ids, ratio, L, 5, 1, V)
        assert not (rows[:n] // L == 0).any() and np.array_equal(masked[0], ids[0])
        live = rows[:n].astype(np.int64)
        assert (np.diff(live) > 0).all()                                  # ascending, hence distinct
        assert np.array_equal(targets[:n], ids.reshape(-1)[live]) and (masked.reshape(-1)[live] == V).all()
        assert ((masked == V) == ((masked != ids))).all()
    # ratio = 1 masks (nearly) every real token; with slots = L every masked position carries a loss
    masked, rows, targets, n = R.cloze_mask(ids, 1.0, L, 5, 1, V)
    assert n == (ids > 0).sum() == (masked == V).sum()
    # truncation keeps the LAST slots drawn positions of a row; the earlier ones stay masked without a loss term
    slots = 3
    m2, rows2, _, n2 = R.cloze_mask(ids, 1.0, slots, 5, 1, V)
    assert np.array_equal(m2, masked)
    for b in range(1, B):
        mine = rows2[:n2][rows2[:n2] // L == b] % L
        drawn = np.nonzero(masked[b] == V)[0]
        assert list(mine) == list(drawn[-slots:])
    # a pure function of (seed, step): equal for equal, different for the next step or another seed
    a = R.cloze_mask(ids, 0.2, 20, 5, 1, V)
    b_ = R.cloze_mask(ids, 0.2, 20, 5, 1, V)
    assert all(np.array_equal(x, y) for x, y in zip(a[:3], b_[:3])) and a[3] == b_[3]
    assert not np.array_equal(a[0], R.cloze_mask(ids, 0.2, 20, 5, 2, V)[0])
    assert not np.array_equal(a[0], R.cloze_mask(ids, 0.2, 20, 6, 1, V)[0])
    # the draw is the complement of the dropout keep mask of the same stream
    from oracle import bsarec_oracle as O
    keep = O.dropout_keep(B * L, R.ratio_f32(0.2), 5, 1, R.CLOZE_SITE).reshape(B, L)
    forced = np.zeros_like(keep)
    for b in range(B):
        if ids[b, -1] > 0 and not ((ids[b] > 0) & ~keep[b]).any():
            forced[b, -1] = True
    assert np.array_equal(a[0] == V, ((ids > 0) & ~keep) | forced)


def test_default_slots_drop_few_positions():
    """The model's default slots = min(L, 2 ceil(ratio L)) = 20 at L = 50, ratio 0.2: full sequences lose almost nothing."""
    B, L = 256, 50
    ids = np.ones((B, L), np.int64)
    drawn = kept = 0
    for step in range(1, 6):
        masked, rows, _, n = R.cloze_mask(ids, 0.2, 20, 42, step, 7)
        drawn += int((masked == 7).sum())
        kept += n
    assert 0.18 <= drawn / (5 * B * L) <= 0.22 and (drawn - kept) / drawn <= 1e-3


def test_patched_oracle_against_finite_differences():
    """fp64, B = 3, L = 7, d = 8, the mask token among the ids: loss_and_grads under the padding-only mask agrees with central
    differences to 1e-6 relative, and position 0's output moves when a LATER token changes (it does not under the causal mask)."""
    from oracle import bsarec_oracle as O
    B, L, d, V = 3, 7, 8, 11
    cfg = O.Config(item_size=V + 1, hidden_size=d, max_seq_length=L, num_hidden_layers=2, num_attention_heads=2, c=3, alpha=0.0,
                   hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0)
    params = {k: v.astype(np.float64) * 5 for k, v in O.init_params(cfg, seed=1).items()}
    rng = np.random.default_rng(2)
    ids = rng.integers(1, V, (B, L))
    ids[0, :3] = 0
    ids[1, 4] = V
    W = rng.normal(0, 1, (B, L, d))
    f = lambda p: float((O.forward(p, cfg, ids, dtype=np.float64)[0][-1] * W).sum())
    with R.bidirectional_oracle():
        d_outs = [np.zeros_like(W), np.zeros_like(W), W]
        _, _, G, outs = O.loss_and_grads(params, cfg, ids, None, dtype=np.float64, d_outs=d_outs, head=R.null_head)
        for key in ("item_embeddings.weight", "item_encoder.blocks.0.layer.attention_layer.query.weight",
                    "item_encoder.blocks.1.feed_forward.dense_1.weight", "position_embeddings.weight"):
            flat = params[key].reshape(-1)
            for i in rng.choice(flat.size, 4, replace=False):
                if key == "position_embeddings.weight" and i >= L * d:
                    continue
                old, eps = flat[i], 1e-5
                flat[i] = old + eps
                up = f(params)
                flat[i] = old - eps
                dn = f(params)
                flat[i] = old
                num, ana = (up - dn) / (2 * eps), G[key].reshape(-1)[i]
                assert abs(num - ana) <= 1e-6 * max(abs(ana), abs(num), 1e-3), (key, i, num, ana)
        ids2 = ids.copy()
        ids2[2, L - 1] = ids[2, L - 1] % (V - 1) + 1
        moved = np.abs(O.forward(params, cfg, ids2, dtype=np.float64)[0][-1][2, 0] - outs[-1][2, 0]).max()
    assert O.attention_mask is not R.padding_mask                 # restored
    causal = np.abs(O.forward(params, cfg, ids2, dtype=np.float64)[0][-1][2, 0] -
                    O.forward(params, cfg, ids, dtype=np.float64)[0][-1][2, 0]).max()
    assert moved > 1e-6 and causal <= 1e-12


NAMES = ("bsarec_plan_set_bidirectional", "bsarec_cloze_mask", "bsarec_cloze_head_workspace_bytes", "bsarec_cloze_head_fwd",
         "bsarec_cloze_head_bwd")


def test_symbols_are_exported_and_bound():
    from bsarec_amd import _lib
    lib = _lib.load()
    for name in NAMES:
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes == _lib.EXPORTS[name][1]
        assert getattr(lib, name).restype == _lib.EXPORTS[name][0]
    n = {k: len(_lib.EXPORTS[k][1]) for k in NAMES}
    assert n["bsarec_cloze_mask"] == 12 and n["bsarec_cloze_head_fwd"] == 15 and n["bsarec_cloze_head_bwd"] == 16
    assert _lib.CLOZE_SITE == R.CLOZE_SITE == 0x434C4F5A
    assert lib.bsarec_abi_version() == 10 and _lib.ABI_VERSION == 10
    assert lib.bsarec_plan_set_bidirectional(None, 1) < 0
    for shape in ((200, 131, 64), (1, 1, 4), (65536, 70001, 256)):
        assert lib.bsarec_cloze_head_workspace_bytes(*shape) == lib.bsarec_ce_head_workspace_bytes(*shape) > 0
    for shape in ((0, 131, 64), (65537, 131, 64), (8, 0, 64), (8, 131, 6), (8, 131, 260)):
        assert lib.bsarec_cloze_head_workspace_bytes(*shape) < 0


LIMITS_C = r"""
#include "bsarec_hip.h"
#include <stdio.h>
#include <math.h>
static long long buf[4096];                                       /* 8-byte aligned, never dereferenced by a refused call */
#define P ((void *)buf)
#define P4 ((void *)((char *)buf + 4))
#define P2 ((void *)((char *)buf + 2))
#define P16 ((void *)(((unsigned long)buf + 64) & ~15ul))
static int bad = 0, cases = 0;
static void neg(int rc, int line) { ++cases; if (rc >= 0) { printf("line %d returned %d\n", line, rc); ++bad; } }
#define NEG(call) neg((int)(call), __LINE__)
#define MASK(ids, B, L, ratio, slots, state, masked, rows, targets, count) \
    bsarec_cloze_mask((const int64_t *)(ids), B, L, ratio, slots, 9, state, (int64_t *)(masked), (int32_t *)(rows), (int64_t *)(targets), (int32_t *)(count), 0)
#define FWD(h, ldh, T, E, R, V, d, rows, targets, count, loss, ws, wsb) \
    bsarec_cloze_head_fwd((const float *)(h), ldh, T, (const float *)(E), R, V, d, (const int32_t *)(rows), (const int64_t *)(targets), (const int32_t *)(count), (float *)(loss), 0, ws, wsb, 0)
#define BWD(h, ldh, T, E, R, V, d, rows, targets, count, g, ws, wsb, dh, dE) \
    bsarec_cloze_head_bwd((const float *)(h), ldh, T, (const float *)(E), R, V, d, (const int32_t *)(rows), (const int64_t *)(targets), (const int32_t *)(count), (const float *)(g), ws, wsb, (float *)(dh), (float *)(dE), 0)
int main(void) {
    long w = bsarec_cloze_head_workspace_bytes(8, 13, 8);
    if (w <= 0 || w != bsarec_ce_head_workspace_bytes(8, 13, 8)) { printf("workspace %ld\n", w); return 2; }
    /* bsarec_cloze_mask: shapes */
    NEG(MASK(P, 0, 8, 0.2f, 2, P, P, P, P, P));      NEG(MASK(P, 65537, 8, 0.2f, 1, P, P, P, P, P));
    NEG(MASK(P, 4, 0, 0.2f, 1, P, P, P, P, P));      NEG(MASK(P, 4, 257, 0.2f, 2, P, P, P, P, P));
    NEG(MASK(P, 4, 8, 0.2f, 0, P, P, P, P, P));      NEG(MASK(P, 4, 8, 0.2f, 9, P, P, P, P, P));
    NEG(MASK(P, 65536, 8, 0.2f, 2, P, P, P, P, P));  NEG(MASK(P, 4097, 16, 0.2f, 16, P, P, P, P, P));
    NEG(MASK(P, 4, 8, -0.1f, 2, P, P, P, P, P));     NEG(MASK(P, 4, 8, 1.5f, 2, P, P, P, P, P));
    NEG(MASK(P, 4, 8, NAN, 2, P, P, P, P, P));
    /* ... pointers: null, then misaligned */
    NEG(MASK(0, 4, 8, 0.2f, 2, P, P, P, P, P));      NEG(MASK(P, 4, 8, 0.2f, 2, 0, P, P, P, P));
    NEG(MASK(P, 4, 8, 0.2f, 2, P, 0, P, P, P));      NEG(MASK(P, 4, 8, 0.2f, 2, P, P, 0, P, P));
    NEG(MASK(P, 4, 8, 0.2f, 2, P, P, P, 0, P));      NEG(MASK(P, 4, 8, 0.2f, 2, P, P, P, P, 0));
    NEG(MASK(P4, 4, 8, 0.2f, 2, P, P, P, P, P));     NEG(MASK(P, 4, 8, 0.2f, 2, P4, P, P, P, P));
    NEG(MASK(P, 4, 8, 0.2f, 2, P, P4, P, P, P));     NEG(MASK(P, 4, 8, 0.2f, 2, P, P, P2, P, P));
    NEG(MASK(P, 4, 8, 0.2f, 2, P, P, P, P4, P));     NEG(MASK(P, 4, 8, 0.2f, 2, P, P, P, P, P2));
    /* bsarec_cloze_head_fwd: the limits of bsarec_ce_head_fwd with B := R, T >= 1, the row list and the count */
    NEG(FWD(P16, 8, 20, P16, 0, 13, 8, P, P, P, P, P16, w));      NEG(FWD(P16, 8, 20, P16, 65537, 13, 8, P, P, P, P, P16, w));
    NEG(FWD(P16, 8, 20, P16, 8, 0, 8, P, P, P, P, P16, w));       NEG(FWD(P16, 8, 20, P16, 8, 13, 6, P, P, P, P, P16, w));
    NEG(FWD(P16, 8, 20, P16, 8, 13, 0, P, P, P, P, P16, w));      NEG(FWD(P16, 8, 20, P16, 8, 13, 260, P, P, P, P, P16, w));
    NEG(FWD(P16, 4, 20, P16, 8, 13, 8, P, P, P, P, P16, w));      NEG(FWD(P16, 10, 20, P16, 8, 13, 8, P, P, P, P, P16, w));
    NEG(FWD(P16, 8, 0, P16, 8, 13, 8, P, P, P, P, P16, w));       NEG(FWD(P16, 8, -3, P16, 8, 13, 8, P, P, P, P, P16, w));
    NEG(FWD(P16, 8, 1L << 31, P16, 8, 13, 8, P, P, P, P, P16, w));
    NEG(FWD(0, 8, 20, P16, 8, 13, 8, P, P, P, P, P16, w));        NEG(FWD(P4, 8, 20, P16, 8, 13, 8, P, P, P, P, P16, w));
    NEG(FWD(P16, 8, 20, 0, 8, 13, 8, P, P, P, P, P16, w));        NEG(FWD(P16, 8, 20, P4, 8, 13, 8, P, P, P, P, P16, w));
    NEG(FWD(P16, 8, 20, P16, 8, 13, 8, 0, P, P, P, P16, w));      NEG(FWD(P16, 8, 20, P16, 8, 13, 8, P2, P, P, P, P16, w));
    NEG(FWD(P16, 8, 20, P16, 8, 13, 8, P, 0, P, P, P16, w));      NEG(FWD(P16, 8, 20, P16, 8, 13, 8, P, P4, P, P, P16, w));
    NEG(FWD(P16, 8, 20, P16, 8, 13, 8, P, P, 0, P, P16, w));      NEG(FWD(P16, 8, 20, P16, 8, 13, 8, P, P, P2, P, P16, w));
    NEG(FWD(P16, 8, 20, P16, 8, 13, 8, P, P, P, 0, P16, w));
    NEG(FWD(P16, 8, 20, P16, 8, 13, 8, P, P, P, P, 0, w));        NEG(FWD(P16, 8, 20, P16, 8, 13, 8, P, P, P, P, P4, w));
    NEG(FWD(P16, 8, 20, P16, 8, 13, 8, P, P, P, P, P16, w - 1));  NEG(FWD(P16, 8, 20, P16, 8, 13, 8, P, P, P, P, P16, 0));
    /* bsarec_cloze_head_bwd: the same, and its own pointers */
    NEG(BWD(P16, 8, 20, P16, 0, 13, 8, P, P, P, P, P16, w, P16, P16));  NEG(BWD(P16, 8, 0, P16, 8, 13, 8, P, P, P, P, P16, w, P16, P16));
    NEG(BWD(P16, 8, 20, P16, 8, 13, 6, P, P, P, P, P16, w, P16, P16));  NEG(BWD(P16, 8, 20, P16, 8, 0, 8, P, P, P, P, P16, w, P16, P16));
    NEG(BWD(P16, 8, 20, P16, 8, 13, 8, 0, P, P, P, P16, w, P16, P16));  NEG(BWD(P16, 8, 20, P16, 8, 13, 8, P, 0, P, P, P16, w, P16, P16));
    NEG(BWD(P16, 8, 20, P16, 8, 13, 8, P, P, 0, P, P16, w, P16, P16));  NEG(BWD(P16, 8, 20, P16, 8, 13, 8, P, P, P, 0, P16, w, P16, P16));
    NEG(BWD(P16, 8, 20, P16, 8, 13, 8, P, P, P, P, P16, w, 0, P16));    NEG(BWD(P16, 8, 20, P16, 8, 13, 8, P, P, P, P, P16, w, P4, P16));
    NEG(BWD(P16, 8, 20, P16, 8, 13, 8, P, P, P, P, P16, w, P16, 0));    NEG(BWD(P16, 8, 20, P16, 8, 13, 8, P, P, P, P, P16, w, P16, P4));
    NEG(BWD(P16, 8, 20, P16, 8, 13, 8, P, P, P, P, P16, w - 1, P16, P16));
    NEG(bsarec_plan_set_bidirectional(0, 1));
    printf("%d cases, %d bad, abi %d, site %x\n", cases, bad, bsarec_abi_version(), BSAREC_CLOZE_SITE);
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
                    "-L", lib_dir, "-lbsarec_hip", f"-Wl,-rpath,{lib_dir}", "-lm"], check=True, capture_output=True)
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")          # no device: a HIP call could not succeed
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.strip().endswith("0 bad, abi 10, site 434c4f5a"), r.stdout
    assert int(r.stdout.split()[0]) == 63                        # every NEG line above ran


def _ns(**kw):
    base = dict(item_size=50, hidden_size=16, max_seq_length=12, batch_size=4, hidden_dropout_prob=0.1,
                attention_probs_dropout_prob=0.1, num_hidden_layers=2, num_attention_heads=2, hidden_act="gelu",
                initializer_range=0.02, seed=1)
    base.update(kw)
    return argparse.Namespace(**base)


def test_flags_tables_and_refusals():
    import bsarec_amd
    from bsarec_amd import BERT4RecModel, main as M, model as Mo
    a = M.parse_args([])
    assert not hasattr(a, "mask_ratio") and not hasattr(a, "bert_mask_slots")          # absent unless given
    a = M.parse_args(["--model_type", "BERT4Rec", "--mask_ratio", "0.2", "--bert_mask_slots", "7"])
    assert a.mask_ratio == 0.2 and a.bert_mask_slots == 7
    for bad in ("0", "1.5", "-0.2", "nan", "x"):
        with pytest.raises(SystemExit):
            M.parse_args(["--mask_ratio", bad])
    assert set(Mo.MODEL_DICT) == {"bsarec", "sasrec", "fmlprec", "duorec", "gru4rec"}     # both pinned tables as they were
    assert set(M.MODEL_DICT) == set(Mo.MODEL_DICT) | {"caser"}
    assert M.SIBLING_MODELS == {"bert4rec": BERT4RecModel} and bsarec_amd.BERT4RecModel is BERT4RecModel
    assert M.model_class("BERT4Rec") is BERT4RecModel and M.model_class("bsarec") is Mo.BSARecModel
    assert M.model_class("Caser") is M.MODEL_DICT["caser"]
    with pytest.raises(KeyError):
        M.model_class("bert5rec")
    args = _ns()
    m = BERT4RecModel(args)
    assert args.item_size == 50 and m.num_items == 50 and m.mask_token == 50             # the caller's args keep V
    assert m.mask_ratio == 0.2 and m.mask_slots == min(12, 2 * 3)
    sd = m.state_dict()
    assert len(sd) == 36 and sd["item_embeddings.weight"].shape == (51, 16)
    assert list(sd) == list(bsarec_amd.SASRecModel(_ns(item_size=51)).state_dict())
    assert m.torch_optim is True and m.needs_negatives is False and m.full_logits is None
    assert m.catalogue_weight().shape == (50, 16) and not m.catalogue_weight().requires_grad
    assert BERT4RecModel(_ns(mask_ratio=1.0, bert_mask_slots=12)).mask_slots == 12
    for kw, msg in ((dict(storage="bf16"), "bf16"), (dict(train_negatives=8), "train_negatives"),
                    (dict(train_lazy_adam=True), "train_lazy_adam"), (dict(mask_ratio=0.0), "mask_ratio"),
                    (dict(mask_ratio=1.01), "mask_ratio"), (dict(mask_ratio=float("nan")), "mask_ratio"),
                    (dict(mask_ratio=-0.5), "mask_ratio"), (dict(bert_mask_slots=0), "bert_mask_slots"),
                    (dict(bert_mask_slots=13), "bert_mask_slots")):
        with pytest.raises(ValueError, match=msg):
            BERT4RecModel(_ns(**kw))
    with pytest.raises(ValueError, match="BERT4Rec: single GPU only"):
        m.check_trainer(args, object())
    m.check_trainer(args, None)
    with pytest.raises(RuntimeError, match="BERT4Rec steps through"):
        m.train_step(None, None)
    with pytest.raises(RuntimeError, match="MI355X"):
        m.calculate_loss(torch.zeros(4, 12, dtype=torch.int64), torch.ones(4, dtype=torch.int64))
