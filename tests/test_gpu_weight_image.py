"""The fragment-ordered fp32 image of the Linear weights (csrc/wimage.h, plan option ``weight_image``).

The fp32 fused block kernels read every weight fragment as ONE coalesced 16-byte-per-lane load from a second copy of the
weights kept in the order of their MFMA operand fragments.  The registers hold what they held before and the MFMAs run in
the same order, so nothing is allowed to change: the tests here ask for bit equality, not for a tolerance.

* host (no GPU): the index map is a bijection for every weight shape and both orientations, and every (tile, k-block)
  fragment is 1 KB contiguous in lane order;
* bit equality: 25 optimisation steps at the C1 shape with dropout on, image on against off;
* currency: the image equals the masters gathered through the index map after every kind of update of the masters.
"""
import argparse
import ctypes as C

import numpy as np
import pytest

# (which, out-features N, in-features K) of the three weight shapes at hidden size 64: query / key / value / dense, dense_1, dense_2
SHAPES = [(0, 64, 64), (4, 256, 64), (5, 64, 256)]
D = 64


def np_offset(col, k, kdim):
    """numpy restatement of wimage_off (csrc/wimage.h)."""
    col, k = np.asarray(col), np.asarray(k)
    return (((col >> 5) * (kdim >> 3) + (k >> 3)) * 64 + (col & 31) + 32 * ((k >> 2) & 1)) * 4 + (k & 3)


def np_weight_base(which, transposed, d=D):
    return (12 * d * d if transposed else 0) + (which if which < 4 else 4 * which - 12) * d * d


def np_index_map(which, transposed, d=D):
    """[N, K] int64: where W[n][k] of weight ``which`` lives inside a layer's image."""
    N, K = (4 * d if which == 4 else d), (4 * d if which == 5 else d)
    n, k = np.meshgrid(np.arange(N), np.arange(K), indexing="ij")
    off = np_offset(k, n, N) if transposed else np_offset(n, k, K)
    return np_weight_base(which, transposed, d) + off


def _lib():
    from bsarec_amd import build as Bd
    from bsarec_amd import _lib as Lb
    Bd.build(force=False, verbose=False)
    return Lb.load()


@pytest.mark.parametrize("which,N,K", SHAPES)
@pytest.mark.parametrize("transposed", [0, 1])
def test_index_map_is_a_bijection_with_contiguous_fragments(which, N, K, transposed):
    lib = _lib()
    off = np.array([[lib.bsarec_wimage_offset(which, transposed, D, n, k) for k in range(K)] for n in range(N)], dtype=np.int64)
    base = np_weight_base(which, transposed)
    # a bijection onto the weight's own N K floats of the image
    assert np.array_equal(np.sort(off.reshape(-1)), base + np.arange(N * K))
    # the numpy restatement the GPU tests gather with is the C function
    assert np.array_equal(off, np_index_map(which, transposed))
    # every fragment = (32-wide tile of fragment columns, 8-deep k-block): lane (j, h) holds k = 8 kb + 4 h + {0..3} of column
    # 32 t + j; the 64 lanes' 16-byte pieces are 1 KB contiguous in lane order.  F: column = n, k = k; T: column = c, k = r.
    cols, kdim = (K, N) if transposed else (N, K)
    at = (lambda col, kk: off[kk, col]) if transposed else (lambda col, kk: off[col, kk])
    starts = set()
    for t in range(cols // 32):
        for kb in range(kdim // 8):
            start = at(32 * t, 8 * kb)
            assert start % 256 == 0
            starts.add(int(start))
            for lane in range(64):
                j, h = lane & 31, lane >> 5
                for s in range(4):
                    assert at(32 * t + j, 8 * kb + 4 * h + s) == start + 4 * lane + s
    assert len(starts) == (cols // 32) * (kdim // 8)


def test_bad_arguments_are_refused():
    lib = _lib()
    assert lib.bsarec_wimage_offset(6, 0, D, 0, 0) == -1 and lib.bsarec_wimage_offset(0, 2, D, 0, 0) == -1
    assert lib.bsarec_wimage_offset(0, 0, D, 64, 0) == -1 and lib.bsarec_wimage_offset(4, 0, D, 255, 63) >= 0
    assert lib.bsarec_wimage_offset(5, 0, D, 0, 255) >= 0 and lib.bsarec_wimage_offset(5, 0, D, 0, 256) == -1


def test_option_is_on_by_default_and_sits_at_the_end_of_the_config():
    from bsarec_amd import _lib as Lb
    assert Lb.default_options()["weight_image"] == 1
    assert Lb.Config._fields_[-1][0] == "weight_image"
    lib = _lib()
    cfg = Lb.Config(256, 50, 64, 2, 2, 3417, 2, 0.9, 1e-12, 0.5, 0.5, 0)
    assert lib.bsarec_wimage_floats(C.byref(cfg)) == 0                  # a zero tail keeps the masters
    cfg.weight_image = 1
    assert lib.bsarec_wimage_floats(C.byref(cfg)) == 2 * 2 * 49152      # 2 layers x 2 orientations x 12 d^2
    for k, v in (("storage", 1), ("x3_products", 1), ("chain_kernels", 1), ("no_fused", 1)):
        setattr(cfg, k, v)
        assert lib.bsarec_wimage_floats(C.byref(cfg)) == 0, k
        setattr(cfg, k, 0)
    cfg.hidden = 128
    assert lib.bsarec_wimage_floats(C.byref(cfg)) == 0                  # not the fused shape


# ---- GPU ---------------------------------------------------------------------------------------
torch = pytest.importorskip("torch")
gpu = pytest.mark.gpu
V, B, L, STEPS = 3417, 256, 50, 25


def _ns(**kw):
    a = argparse.Namespace(item_size=V, hidden_size=64, max_seq_length=L, batch_size=B, hidden_dropout_prob=0.5,
                           attention_probs_dropout_prob=0.5, num_hidden_layers=2, num_attention_heads=2,
                           hidden_act="gelu", initializer_range=0.02, c=3, alpha=0.9, seed=42)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _model(image, **kw):
    from bsarec_amd import BSARecModel
    opts = dict(kw.pop("plan_options", {}), weight_image=image)
    torch.manual_seed(3)
    m = BSARecModel(_ns(plan_options=opts, **kw)).cuda()
    m.configure_adam(lr=1e-3)
    m.set_seed(1234)
    m.train()
    return m


def _table(n, seed=0):
    rng = np.random.default_rng(seed)
    ids = rng.integers(1, V, size=(n, L)).astype(np.int64)
    for r in range(n):
        ids[r, :rng.integers(0, L)] = 0
    return torch.from_numpy(ids).cuda(), torch.from_numpy(rng.integers(1, V, size=n).astype(np.int64)).cuda()


def _indexed_steps(m, steps, seed=0):
    """``steps`` x bsarec_train_step_indexed (the fused reduce + Adam launch) over a table of that many batches."""
    table, ans = _table(steps * B, seed)
    perm = torch.randperm(steps * B, generator=torch.Generator().manual_seed(seed)).cuda()
    cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
    loss = None
    for _ in range(steps):
        loss = m.train_step_indexed(table, ans, perm, cursor, B).clone()
    torch.cuda.synchronize()
    assert int(cursor.item()) == steps * B
    return loss


def _assert_image_current(m):
    """Both images of every layer, read back, equal the masters gathered through the index map."""
    torch.cuda.synchronize()
    assert m._wimage is not None, "this model's plans keep no fragment image"
    img = m._wimage.cpu()
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    names = ["layer.attention_layer.query", "layer.attention_layer.key", "layer.attention_layer.value",
             "layer.attention_layer.dense", "feed_forward.dense_1", "feed_forward.dense_2"]
    per_layer = 24 * D * D
    assert img.numel() == m.args.num_hidden_layers * per_layer
    for l in range(m.args.num_hidden_layers):
        for which, name in enumerate(names):
            w = sd[f"item_encoder.blocks.{l}.{name}.weight"]
            for transposed in (0, 1):
                idx = torch.from_numpy(np_index_map(which, transposed)) + l * per_layer
                assert torch.equal(img[idx], w), (l, name, "T" if transposed else "F")


@gpu
@pytest.mark.parametrize("no_prune_top", [0, 1], ids=["pruned_top", "full_top"])
@pytest.mark.parametrize("heads", [2, 1])
def test_training_is_bit_identical_with_and_without_the_image(heads, no_prune_top):
    out = []
    for image in (1, 0):
        m = _model(image, num_attention_heads=heads, plan_options={"no_prune_top": no_prune_top})
        loss = _indexed_steps(m, STEPS)
        assert (m._wimage is not None) == bool(image)
        if image:
            _assert_image_current(m)                      # the fused Adam's in-kernel stores (reduce_adam_kernel)
        out.append((loss.cpu(), {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}))
    (la, sa), (lb, sb) = out
    assert torch.isfinite(la).all() and torch.equal(la, lb), (la, lb)
    assert set(sa) == set(sb)
    for k in sa:
        assert torch.equal(sa[k], sb[k]), k


@gpu
def test_image_stays_current_under_every_writer_of_the_masters():
    from bsarec_amd import _lib as Lb
    m = _model(1)
    _indexed_steps(m, 3)
    _assert_image_current(m)
    # load_state_dict of perturbed weights, then one forward
    sd = {k: v.detach().clone() for k, v in m.state_dict().items()}
    g = torch.Generator(device="cpu").manual_seed(5)
    for k in sd:
        sd[k] = sd[k] + 0.01 * torch.randn(sd[k].shape, generator=g).to(sd[k].device)
    m.load_state_dict(sd)
    ids, ans = _table(B, seed=9)
    m.eval()
    m.full_logits(ids)
    m.train()
    _assert_image_current(m)
    # the eager step (bsarec_train_step: backward, then adam_kernel as a launch of its own)
    m.train_step(ids, ans)
    _assert_image_current(m)
    # one adam_kernel step called directly, the way the data-parallel step and bench.py's peer-to-peer probe call it
    plan = m._plan(B)
    m._garena.normal_()
    a = m._adam
    ad = Lb.Adam(m._arena.data_ptr(), m._garena.data_ptr(), a["m"].data_ptr(), a["v"].data_ptr(), m._numel,
                 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, None, 0)
    ad.n_grad_srcs = 1
    ad.grad_srcs[0] = m._garena.data_ptr()
    ad.wimage_plan = plan.handle
    before = m._arena.clone()
    Lb.check(Lb.load().bsarec_adam_step(C.byref(ad), m._state.data_ptr(), torch.cuda.current_stream().cuda_stream),
             "bsarec_adam_step")
    torch.cuda.synchronize()
    assert not torch.equal(before, m._arena)
    _assert_image_current(m)
    # ... and through the model's own plan-less Adam (what Trainer's data-parallel step runs)
    m._garena.normal_()
    m.adam_step()
    _assert_image_current(m)


@gpu
@pytest.mark.parametrize("path", ["eager", "indexed"])
def test_image_stays_current_under_lazy_adam(path):
    """``train_negatives`` + ``train_lazy_adam``: lazy_adam_kernel's dense blocks update the block weights."""
    m = _model(1, train_negatives=256, train_lazy_adam=True)
    before = m._arena.clone()
    if path == "indexed":
        _indexed_steps(m, 3)
    else:
        for s in range(3):
            ids, ans = _table(B, seed=20 + s)
            m.train_step(ids, ans)
    torch.cuda.synchronize()
    assert not torch.equal(before, m._arena)
    _assert_image_current(m)


@gpu
def test_plans_of_one_model_share_the_image():
    """An evaluation plan of another batch size reads the image the training plan's Adam keeps current."""
    m = _model(1)
    _indexed_steps(m, 2)
    ids, _ = _table(32, seed=4)
    m.eval()
    a = m.full_logits(ids).clone()
    m.train()
    _indexed_steps(m, 2, seed=1)
    m.eval()
    ref = _model(0)
    ref.load_state_dict(m.state_dict())
    ref.eval()
    assert torch.equal(m.full_logits(ids), ref.full_logits(ids))
    assert not torch.equal(a, m.full_logits(ids))
