"""The weight-gradient launch of the fused shape (dw_direct.h) at the edges of its token decomposition: slab slices that
are empty, partial or whole, quarters that end inside a k-block, the four waves' shared reduction of a slab tile (output
rows past M, the bias row), the pruned top block's small problems, fp32 and bf16 storage (8- and 16-row k-blocks).

  * one training step at B in {1, 3, 37, 256, 1024} x L in {7, 50, 64} x {fp32, bf16 storage}, pruned / full top block and
    1 / 2 heads spread over the set so that every (storage, prune, heads) combination occurs: loss and all 42 gradients
    against ``oracle.loss_and_grads`` at the gates of tests/test_gpu_parity.py (fp32, fused path: 5e-6 on the loss,
    2e-4 rel-L2 per gradient, key.bias <= 1e-6) and tests/test_gpu_bf16.py (LOSS_GATE, GRAD_GATE, key.bias <= 1e-4).
    ``oracle_case`` is importable without a GPU: every case's oracle gradients were checked finite and not identically
    zero (key.bias, whose true gradient is zero, aside).
  * the same step twice from the same state: bit-identical gradients, dense weights and item table, fp32 and bf16 storage,
    and for other slab-slice counts than the default.
"""
import argparse

import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

V = 131
BS, LS = (1, 3, 37, 256, 1024), (7, 50, 64)
CASES = []
for ib, B in enumerate(BS):
    for il, L in enumerate(LS):
        for st, storage in enumerate(("f32", "bf16")):
            n = ib + il + st
            CASES.append((B, L, storage, n % 2, 1 + (n // 2) % 2))        # prune, heads
assert {c[2:] for c in CASES} == {(s, p, h) for s in ("f32", "bf16") for p in (0, 1) for h in (1, 2)}


def oracle_case(B, L, heads):
    """Parameters, batch and oracle results of one case (CPU only)."""
    from oracle import bsarec_oracle as O
    cfg = O.Config(item_size=V, hidden_size=64, max_seq_length=L, num_hidden_layers=2, num_attention_heads=heads,
                   c=5, alpha=0.7, hidden_dropout_prob=0.4, attention_probs_dropout_prob=0.3)
    params = O.init_params(cfg, seed=heads + L)
    rng = np.random.default_rng(1000 * L + B)
    for k in params:
        if k.endswith(".bias"):
            params[k] = (rng.standard_normal(params[k].shape) * 0.05).astype(np.float32)
        elif "LayerNorm.weight" in k:
            params[k] = (1 + rng.standard_normal(params[k].shape) * 0.1).astype(np.float32)
    ids = np.zeros((B, L), dtype=np.int64)
    for b in range(B):
        n = L if b == 0 else int(rng.integers(0, L + 1))
        if n:
            ids[b, L - n:] = rng.integers(1, V, size=n)
    ans = rng.integers(1, V, size=B).astype(np.int64)
    oloss, _, G, _ = O.loss_and_grads(params, cfg, ids, ans, O.DropoutSpec(True, 77, 1))
    return cfg, params, ids, ans, oloss, G


def _model(cfg, params, storage):
    from bsarec_amd import BSARecModel
    a = argparse.Namespace(
        item_size=cfg.item_size, hidden_size=cfg.hidden_size, max_seq_length=cfg.max_seq_length, batch_size=256,
        hidden_dropout_prob=cfg.hidden_dropout_prob, attention_probs_dropout_prob=cfg.attention_probs_dropout_prob,
        num_hidden_layers=cfg.num_hidden_layers, num_attention_heads=cfg.num_attention_heads, hidden_act="gelu",
        initializer_range=cfg.initializer_range, c=cfg.c, alpha=cfg.alpha, seed=42)
    if storage == "bf16":
        a.storage = "bf16"
    m = BSARecModel(a)
    m.load_state_dict({k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in params.items()})
    m = m.cuda()
    m.train()
    return m


@pytest.mark.parametrize("B,L,storage,prune,heads", CASES)
def test_training_step_gradients_vs_oracle(B, L, storage, prune, heads):
    from bsarec_amd import _lib as Lb
    from test_gpu_bf16 import GRAD_GATE, LOSS_GATE
    old = Lb.set_default_options(no_prune_top=1 - prune)
    try:
        cfg, params, ids, ans, oloss, G = oracle_case(B, L, heads)
        model = _model(cfg, params, storage)
        model.set_seed(77)
        loss = model.calculate_loss(torch.from_numpy(ids).cuda(), torch.from_numpy(ans).cuda(), None, None, None)
        loss.backward()
        torch.cuda.synchronize()
        plan = model._plan(B)
        assert Lb.load().bsarec_plan_is_fused(plan.handle) > 0
        bf = storage == "bf16"
        assert bool(plan.bf16) == bf
        loss_gate, grad_gate, kb_gate = (LOSS_GATE, GRAD_GATE, 1e-4) if bf else (5e-6, 2e-4, 1e-6)
        loss_err = abs(loss.item() - oloss) / abs(oloss)
        got = model.grad_views()
        assert set(got) == set(G)
        errs = {}
        for k, r in G.items():
            g = got[k].cpu().numpy()
            assert np.isfinite(g).all(), k
            if k.endswith("key.bias"):                     # true gradient is zero
                assert np.abs(g).max() <= kb_gate, (k, np.abs(g).max())
                continue
            assert np.abs(r).max() > 0, k
            errs[k] = rel_l2(g, r)
        worst = max(errs, key=errs.get)
        print(f"B={B} L={L} {storage} prune={prune} heads={heads}: loss rel {loss_err:.2e}, worst gradient {errs[worst]:.2e} ({worst})")
        assert loss_err <= loss_gate, loss_err
        assert errs[worst] <= grad_gate, {k: v for k, v in errs.items() if v > grad_gate}
    finally:
        Lb.set_default_options(**old)


@pytest.mark.parametrize("splits", [0, 7, 40, 64])
@pytest.mark.parametrize("storage", ["f32", "bf16"])
def test_same_step_twice_is_bit_identical(storage, splits):
    """Fixed-order sums of quarters and slabs, integer row atomics for the item table: a step is reproducible bit for bit."""
    from bsarec_amd import _lib as Lb
    old = Lb.set_default_options(splits=splits)
    try:
        cfg, params, ids, ans, _, _ = oracle_case(37, 50, 2)
        runs = []
        for _ in range(2):
            model = _model(cfg, params, storage)
            model.set_seed(77)
            loss = model.calculate_loss(torch.from_numpy(ids).cuda(), torch.from_numpy(ans).cuda(), None, None, None)
            loss.backward()
            torch.cuda.synchronize()
            runs.append({k: v.cpu().numpy().copy() for k, v in model.grad_views().items()})
            runs[-1]["loss"] = np.float32(loss.item())
        for k in runs[0]:
            np.testing.assert_array_equal(runs[0][k], runs[1][k], err_msg=k)
        assert np.abs(runs[0]["item_embeddings.weight"]).max() > 0
    finally:
        Lb.set_default_options(**old)
