"""Keep bits of the dropout masks (csrc/drop_bits.h, plan option ``drop_bits``): the forward block kernels leave
one bit per mask element, the backward reads the bits instead of evaluating Philox again.

* host only: the index map is a bijection into the layer's buffer, sites do not overlap, the numpy restatement used below is
  the library's map;
* GPU: the bits a training forward leaves are the oracle's keep masks; training with the option on and off is the same bit
  for bit (loss, every state_dict tensor, every activation a forward saves)."""
import argparse
import ctypes as C
import itertools

import numpy as np
import pytest

SLOTS = {"embed": 0, "f": 1, "o": 2, "ff": 3}


# ---- numpy restatement of drop_bits.h ------------------------------------------------------------
def hidden_bit(slot, T, token, c):
    return (((slot * T + token) * 16) + c // 4) * 8 + (c & 3)


def attn_bit(T, heads, b, head, query, key):
    word = (((b * heads + head) * 2 + key // 32) * 2 + ((key // 4) & 1)) * 64 + query
    return (4 * T * 16 + 2 * word) * 8 + 4 * ((key // 8) & 3) + (key & 3)


def layer_bytes(B, L, heads):
    return 4 * B * L * 16 + B * heads * 256 * 2


def _lib():
    from bsarec_amd import _lib as Lb
    return Lb.load()


@pytest.mark.parametrize("L", [1, 7, 32, 50, 64])
def test_index_map_is_a_bijection_and_sites_do_not_overlap(L):
    lib = _lib()
    B, heads = 3, 2
    T = B * L
    nbits = layer_bytes(B, L, heads) * 8
    tok, col = np.meshgrid(np.arange(T), np.arange(64), indexing="ij")
    seen = np.zeros(nbits, dtype=np.int32)
    for slot in range(4):
        idx = hidden_bit(slot, T, tok, col).reshape(-1)
        assert idx.min() >= slot * T * 128 and idx.max() < (slot + 1) * T * 128          # a slot's bytes are its own
        np.add.at(seen, idx, 1)
        for t, c in ((0, 0), (T - 1, 63), (T // 2, 5)):
            assert lib.bsarec_drop_bits_hidden_bit(slot, T, t, c) == hidden_bit(slot, T, t, c)
    b, h, q, k = np.meshgrid(np.arange(B), np.arange(heads), np.arange(L), np.arange(L), indexing="ij")
    idx = attn_bit(T, heads, b, h, q, k).reshape(-1)
    assert idx.min() >= 4 * T * 128 and idx.max() < nbits                                # behind the hidden slots, inside the buffer
    np.add.at(seen, idx, 1)
    assert seen.max() == 1                                                               # no two elements share a bit
    assert int(seen.sum()) == 4 * T * 64 + B * heads * L * L
    # every element through the library's own functions at the shape the GPU test reads back
    if L == 50:
        for slot in range(4):
            got = np.array([[lib.bsarec_drop_bits_hidden_bit(slot, T, t, c) for c in range(64)] for t in range(0, T, 7)])
            assert np.array_equal(got, hidden_bit(slot, T, tok, col)[::7])
        got = np.array([lib.bsarec_drop_bits_attn_bit(T, heads, bb, hh, qq, kk)
                        for bb, hh, qq, kk in itertools.product(range(B), range(heads), range(0, L, 3), range(L))])
        assert np.array_equal(got, attn_bit(T, heads, b, h, q, k)[:, :, ::3].reshape(-1))
    # bad arguments
    assert lib.bsarec_drop_bits_hidden_bit(4, T, 0, 0) == -1 and lib.bsarec_drop_bits_hidden_bit(0, T, T, 0) == -1
    assert lib.bsarec_drop_bits_hidden_bit(0, T, 0, 64) == -1 and lib.bsarec_drop_bits_attn_bit(T, heads, 0, heads, 0, 0) == -1
    assert lib.bsarec_drop_bits_attn_bit(T, heads, 0, 0, 64, 0) == -1 and lib.bsarec_drop_bits_attn_bit(T, heads, 0, 0, 0, 64) == -1


def test_option_is_on_by_default_and_sized_by_the_library():
    from bsarec_amd import _lib as Lb
    lib = _lib()
    assert Lb.default_options()["drop_bits"] == 1 and "drop_bits" not in Lb.OPTION_FIELDS      # a plan setter, not a config field
    cfg = Lb.Config(3, 50, 64, 2, 2, 97, 2, 0.9, 1e-12, 0.5, 0.5, 0)
    assert lib.bsarec_drop_bits_bytes(C.byref(cfg)) == layer_bytes(3, 50, 2)
    for k, v in (("x3_products", 1), ("chain_kernels", 1), ("no_fused", 1), ("separate_embed", 1)):
        setattr(cfg, k, v)
        assert lib.bsarec_drop_bits_bytes(C.byref(cfg)) == 0, k
        setattr(cfg, k, 0)
    cfg.storage = 1
    assert lib.bsarec_drop_bits_bytes(C.byref(cfg)) == layer_bytes(3, 50, 2)
    cfg.hidden = 128
    assert lib.bsarec_drop_bits_bytes(C.byref(cfg)) == 0                  # not the fused shape


# ---- GPU ---------------------------------------------------------------------------------------
torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu
V, B, STEPS = 97, 3, 5


def _ns(L, heads, layers, p, **kw):
    a = argparse.Namespace(item_size=V, hidden_size=64, max_seq_length=L, batch_size=B, hidden_dropout_prob=p,
                           attention_probs_dropout_prob=p, num_hidden_layers=layers, num_attention_heads=heads,
                           hidden_act="gelu", initializer_range=0.02, c=3, alpha=0.9, seed=42, lr=1e-3, adam_beta1=0.9,
                           adam_beta2=0.999, weight_decay=0.0, no_cuda=False, log_freq=1)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _ids(n, L, seed):
    rng = np.random.default_rng(seed)
    ids = rng.integers(1, V, size=(n, L)).astype(np.int64)
    for r in range(n):
        ids[r, :rng.integers(0, L)] = 0                               # left padding of every length
    return ids, rng.integers(1, V, size=n).astype(np.int64)


def _saved(m, plan):
    """Every activation a forward keeps for the backward: the workspace from the embedding output up to the logits."""
    from bsarec_amd import _lib as Lb
    lo = plan.lib.bsarec_buffer_offset(plan.handle, Lb.BUF_LAYER_OUT, 0)
    hi = plan.lib.bsarec_buffer_offset(plan.handle, Lb.BUF_LOGITS, 0)
    assert 0 <= lo < hi
    return plan.ws[lo:hi].cpu()


def _run(on, L, heads, arch, storage, p):
    from bsarec_amd import BSARecModel
    from bsarec_amd.data import DeviceBatches
    from bsarec_amd.trainer import Trainer
    layers = 1 if arch == "one_layer" else 2
    opts = {"drop_bits": on, "storage": storage, "no_prune_top": int(arch == "full_top")}
    args = _ns(L, heads, layers, p, plan_options=opts)
    torch.manual_seed(3)
    m = BSARecModel(args)
    ids, ans = _ids(B * STEPS, L, seed=L + heads)
    dl = DeviceBatches(np.arange(B * STEPS, dtype=np.int64), ids, ans, B, torch.device("cuda"), shuffle=False)
    tr = Trainer(m, dl, None, None, args)
    m = tr.model
    m.set_seed(1234)
    m.train()
    # one forward of the loss path, and what it saved
    plan = m._run_forward(dl.inputs[:B], train=True, new_step=True, last_only=True)
    torch.cuda.synchronize()
    saved = _saved(m, plan)
    from bsarec_amd import _lib as Lb
    assert plan.options["drop_bits"] == on and plan.lib.bsarec_buffer_offset(plan.handle, Lb.BUF_DROP_BITS, 0) >= 0
    # five optimisation steps, graph replay
    perm = torch.arange(B * STEPS, dtype=torch.int64, device="cuda")
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    loss = tr.indexed_steps(dl, perm, cursor, None, STEPS).clone()
    torch.cuda.synchronize()
    assert int(cursor.item()) == B * STEPS and tr.graphs_built() > 0
    return loss.cpu(), {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}, saved


@gpu
@pytest.mark.parametrize("p", [0.5, 0.0], ids=["p0.5", "p0"])
@pytest.mark.parametrize("storage", [0, 1], ids=["fp32", "bf16"])
@pytest.mark.parametrize("arch", ["pruned_top", "full_top", "one_layer"])
@pytest.mark.parametrize("heads", [1, 2])
@pytest.mark.parametrize("L", [50, 32, 7])
def test_training_is_bit_identical_with_and_without_the_bits(L, heads, arch, storage, p):
    (loss1, sd1, saved1), (loss0, sd0, saved0) = (_run(on, L, heads, arch, storage, p) for on in (1, 0))
    assert torch.isfinite(loss1).all() and torch.equal(loss1, loss0)
    for k in sd1:
        assert torch.equal(sd1[k], sd0[k]), k
    assert saved1.numel() == saved0.numel()           # (the bits live behind the saved activations: the same carve up to them)
    assert torch.equal(saved1, saved0)


def _bits(plan, layer, nbytes):
    from bsarec_amd import _lib as Lb
    off = plan.lib.bsarec_buffer_offset(plan.handle, Lb.BUF_DROP_BITS, layer)
    assert off >= 0
    return np.unpackbits(plan.ws[off:off + nbytes].cpu().numpy(), bitorder="little").astype(bool)


@gpu
@pytest.mark.parametrize("storage", [0, 1], ids=["fp32", "bf16"])
def test_the_bits_are_the_oracle_keep_masks(storage):
    from bsarec_amd import BSARecModel, _lib as Lb
    from oracle import bsarec_oracle as O
    L, heads, layers, p = 50, 2, 2, 0.5
    T, Lp = B * L, 52
    nbytes = layer_bytes(B, L, heads)
    torch.manual_seed(3)
    m = BSARecModel(_ns(L, heads, layers, p, plan_options={"storage": storage})).cuda()
    m.set_seed(1234)
    m.train()
    ids = torch.from_numpy(_ids(B, L, seed=5)[0]).cuda()
    tok, col = np.meshgrid(np.arange(T), np.arange(64), indexing="ij")
    b, h, q, k = np.meshgrid(np.arange(B), np.arange(heads), np.arange(L), np.arange(L), indexing="ij")
    for last_only in (False, True):                                   # every row of every layer; then the one-row top block
        plan = m._run_forward(ids, train=True, new_step=True, last_only=last_only)
        torch.cuda.synchronize()
        assert Lb.load().bsarec_drop_bits_bytes(C.byref(plan.cfg)) == nbytes
        seed, step = int(m._state[0].item()), int(m._state[1].item())
        for l in range(layers):
            bits = _bits(plan, l, nbytes)
            top_row = last_only and l == layers - 1                   # the pruned top block holds row / query L - 1 only
            rows = (tok % L == L - 1) if top_row else np.ones_like(tok, dtype=bool)
            for name, site in (("embed", 0), ("f", 1 + 4 * l), ("o", 3 + 4 * l), ("ff", 4 + 4 * l)):
                if name == "embed" and l > 0:
                    continue
                keep = O.dropout_keep(T * 64, p, seed, step, site).reshape(T, 64)
                got = bits[hidden_bit(SLOTS[name], T, tok, col)]
                assert np.array_equal(got[rows], keep[rows]), (last_only, l, name)
                assert 0.4 < keep.mean() < 0.6
            keep = O.dropout_keep(B * heads * L * Lp, p, seed, step, 2 + 4 * l).reshape(B, heads, L, Lp)[..., :L]
            got = bits[attn_bit(T, heads, b, h, q, k)]
            sel = (q == L - 1) if top_row else np.ones_like(q, dtype=bool)
            assert np.array_equal(got[sel], keep[sel]), (last_only, l, "attention")
