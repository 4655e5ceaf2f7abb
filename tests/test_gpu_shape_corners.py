"""The block stack against the float64 oracle at the corners of what ``check_cfg`` admits (include/bsarec_hip.h): hidden sizes
inside a tile class (68, 100, 132, 252), head widths 4 / 12 / 20 / 36 / 44, reduction lengths that are no power of two, sequence
lengths 1, 2, just above a tile class (65, 129) and at the limit (255, 256), every cutoff 1 .. 8 of the fused kernels, the
boundaries ``cutoff_bins == L/2``, ``== L/2 + 1`` and ``cutoff_bins * hidden == 8192``, and the d = 64 configurations that leave
the fused path without notice (8 or 16 heads, L = 65, cutoff_bins = 9).

What differs from the other parity tests:
  * the reference is ``oracle.loss_and_grads(dtype=np.float64)``; the float32 oracle is run as well and its distance from the
    float64 one, per gradient tensor (``n_k``), is the noise floor a gradient gate may not go below;
  * ``query.weight`` / ``key.weight`` are drawn N(0, 1.2 / sqrt(d)), so the scores have a std near 1.4 and the softmax is far
    from uniform: an error in the mask, the row max or the 1 / sqrt(dh) scale moves the result.

Gates of the fp32 cases, all against the float64 oracle: loss 5e-6 relative; layer outputs rel-L2 <= 2e-5 and max abs <= 1e-3 on
every row the variant produces; gradient of tensor k rel-L2 <= max(2e-4, 4 n_k) (two independent fp32 evaluations add in
quadrature, and the kernels sum in split-K / MFMA order, not numpy's pairwise order); a tensor whose float64 gradient is exactly
zero (key.bias; query.*, key.weight at L = 1): max |g| <= 1e-6; d sqrt_beta where the filter keeps the whole spectrum
(cutoff_bins == L // 2 + 1: x - low is rounding error): both sides <= 1e-5 absolute.  The bf16 cases keep ``init_params``' own
query / key weights and the gates of tests/test_gpu_bf16.py, which were set with those.

Every case prints one ``shape_corners`` line with its worst errors before it asserts (profiles/shape_corners_errors.txt)."""
import numpy as np
import pytest

from conftest import rel_l2
from test_gpu_parity import build_model

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

V, SEED = 37, 77

# (d, heads, L, B, c, cutoff_bins, layers)
GENERIC = [
    (4, 1, 1, 3, 3, 1, 2),          # every minimum at once; a single key; Lp = 4
    (4, 1, 2, 70, 3, 2, 2),         # T = 140 spans three 64-row tiles; whole spectrum kept
    (20, 5, 7, 5, 5, 3, 2),         # K = dh = 4 below one k-block; d no power of two
    (36, 3, 33, 3, 9, 5, 2),        # dh = 12; Lp = 36
    (64, 8, 50, 5, 5, 3, 2),        # the benchmark shape pushed off the fused path by the heads
    (64, 16, 50, 3, 5, 3, 2),       # the same with dh = 4
    (64, 2, 65, 3, 5, 3, 2),        # pushed off by L; Lp = 68 opens the 128-wide softmax / dS tiles
    (64, 2, 50, 5, 17, 9, 2),       # pushed off by cutoff_bins = FUSED_MAX_CB + 1
    (68, 1, 65, 3, 7, 4, 2),        # first d in the 128-wide LayerNorm tile
    (100, 5, 100, 3, 21, 11, 2),    # interior of the 128 class; K = 100 = 3 k-tiles + 4
    (132, 3, 129, 2, 15, 8, 2),     # first d and first Lp in the 256-wide tiles
    (252, 7, 255, 2, 31, 16, 1),    # last d and an odd L below the limits
    (256, 4, 256, 2, 63, 32, 1),    # both limits; cutoff_bins * d = 8192 exactly
    (256, 64, 127, 2, 63, 32, 1),   # 64 heads of width 4 at the widest d
]

# d = 64: (heads, L, B, c, cutoff_bins, layers)
FUSED = [
    (2, 50, 5, 1, 1, 2),
    (2, 50, 5, 7, 4, 2),
    (4, 64, 3, 11, 6, 2),
    (1, 64, 3, 13, 7, 2),
    (2, 64, 3, 15, 8, 2),
    (2, 50, 21, 15, 8, 3),
    (2, 16, 4, 14, 8, 2),           # cutoff_bins = L/2: the last bin below Nyquist
    (2, 14, 6, 15, 8, 2),           # cutoff_bins = L/2 + 1: whole spectrum, Nyquist included
    (2, 15, 6, 15, 8, 2),           # the same with an odd L: no Nyquist bin
    (1, 1, 3, 1, 1, 2),
    (4, 3, 5, 1, 1, 2),
]
# the register-chain forward kernel keeps re[FUSED_MAX_CB] in registers, x3 splits every product: cutoffs 1, 7, 8 at L >= 50
FUSED_VARIANT_CASES = [c for c in FUSED if c[4] in (1, 7, 8) and c[1] >= 50]


def _gid(c):
    return "d%d_h%d_L%d_B%d_c%d_n%d" % (c[0], c[1], c[2], c[3], c[4], c[6])


def _fid(c):
    return _gid((64,) + tuple(c))


_REF = {}


def _zero_grad(k, ref):
    """key.bias (softmax is shift invariant: its true gradient is zero, the oracle's is rounding noise), and any tensor whose float64
    gradient is exactly zero (query.*, key.weight at L = 1: a single key)."""
    return k.endswith("key.bias") or not np.any(ref)


def _reference(d, heads, L, B, c, layers, act="gelu", sharp=True):
    """Parameters, the ragged batch and both oracle runs of a case; computed once, shared by every variant, never modified."""
    key = (d, heads, L, B, c, layers, act, sharp)
    if key in _REF:
        return _REF[key]
    from oracle import bsarec_oracle as O
    cfg = O.Config(item_size=V, hidden_size=d, max_seq_length=L, num_hidden_layers=layers, num_attention_heads=heads, c=c,
                   alpha=0.7, hidden_dropout_prob=0.3, attention_probs_dropout_prob=0.2, hidden_act=act)
    params = O.init_params(cfg, seed=d + heads + L)
    rng = np.random.default_rng(1000 * d + 10 * L + c)
    for k in params:
        if k.endswith(".bias"):
            params[k] = (rng.standard_normal(params[k].shape) * 0.05).astype(np.float32)
        elif "LayerNorm.weight" in k:
            params[k] = (1 + rng.standard_normal(params[k].shape) * 0.1).astype(np.float32)
        elif sharp and (k.endswith("query.weight") or k.endswith("key.weight")):
            params[k] = (rng.standard_normal(params[k].shape) * (1.2 / np.sqrt(d))).astype(np.float32)
    ids = np.zeros((B, L), dtype=np.int64)
    for b in range(B):                     # sequence 0 all padding, sequence 1 full, the rest ragged
        n = 0 if b == 0 else (L if b == 1 else int(rng.integers(1, L + 1)))
        if n:
            ids[b, L - n:] = rng.integers(1, V, size=n)
    ans = rng.integers(1, V, size=B).astype(np.int64)
    drop = O.DropoutSpec(True, SEED, 1)
    loss64, logits64, G64, outs64 = O.loss_and_grads(params, cfg, ids, ans, drop, dtype=np.float64)
    loss32, _, G32, outs32 = O.loss_and_grads(params, cfg, ids, ans, drop, dtype=np.float32)
    noise = {k: rel_l2(G32[k], G64[k]) for k in G64 if not _zero_grad(k, G64[k])}
    for a in list(G64.values()) + list(outs64) + [logits64]:
        a.setflags(write=False)
    ref = dict(cfg=cfg, params=params, ids=ids, ans=ans, loss=float(loss64), logits=logits64, G=G64, outs=outs64, noise=noise)
    # the reference alone stays inside every gate, so a miss is the kernels'
    assert abs(float(loss32) - ref["loss"]) <= 5e-6 * abs(ref["loss"])
    assert all(rel_l2(a, b) <= 2e-5 for a, b in zip(outs32, outs64))
    _REF[key] = ref
    return ref


def _run(ref, **kw):
    cfg, ids, ans = ref["cfg"], ref["ids"], ref["ans"]
    model = build_model(cfg, ref["params"], hidden_act=cfg.hidden_act, **kw)
    model.train()
    model.set_seed(SEED)
    loss = model.calculate_loss(torch.from_numpy(ids).cuda(), torch.from_numpy(ans).cuda(), None, None, None)
    loss.backward()
    torch.cuda.synchronize()
    assert int(model._state[1].item()) == 1
    return model, model._plan(ids.shape[0]), loss.item()


def _layer_outputs(plan, ref, pruned):
    from bsarec_amd import _lib as Lb
    cfg = ref["cfg"]
    B, L = ref["ids"].shape
    N = cfg.num_hidden_layers
    for l in range(N + 1):
        g = plan.view(Lb.BUF_LAYER_OUT, l, (B, L, cfg.hidden_size)).float().cpu().numpy()
        r = ref["outs"][l]
        if pruned and l == N:               # the one-row top block: only position L-1 of the last layer exists
            g, r = g[:, -1], r[:, -1]
        assert np.isfinite(g).all(), l
        yield l, g, r, (ref["ids"] > 0) if not (pruned and l == N) else (ref["ids"][:, -1] > 0)


def _check_fp32(tag, d, heads, L, B, c, cb, layers, fused, act="gelu", **opts):
    from bsarec_amd import _lib as Lb
    ref = _reference(d, heads, L, B, c, layers, act)
    old = Lb.set_default_options(**opts)
    try:
        model, plan, loss = _run(ref)
        assert plan.cfg.cutoff_bins == cb == ref["cfg"].cutoff_bins
        assert plan.lib.bsarec_plan_is_fused(plan.handle) == fused
        pruned = bool(fused) and layers >= 2 and not opts.get("no_prune_top", 0)
        loss_err = abs(loss - ref["loss"]) / abs(ref["loss"])
        out_rel = out_abs = 0.0
        for l, g, r, _ in _layer_outputs(plan, ref, pruned):
            out_rel, out_abs = max(out_rel, rel_l2(g, r)), max(out_abs, float(np.abs(g - r).max()))
        whole = cb == L // 2 + 1
        G, noise = ref["G"], ref["noise"]
        got = {k: v.cpu().numpy() for k, v in model.grad_views().items()}
        assert set(got) == set(G)
        errs, zeros, beta = {}, {}, {}
        for k, r in G.items():
            assert np.isfinite(got[k]).all(), k
            if whole and k.endswith("sqrt_beta"):
                beta[k] = max(float(np.abs(got[k]).max()), float(np.abs(r).max()))
            elif _zero_grad(k, r):
                zeros[k] = float(np.abs(got[k]).max())
            else:
                errs[k] = rel_l2(got[k], r)
        wk = max(errs, key=lambda k: errs[k] / max(2e-4, 4 * noise[k]))
        print(f"shape_corners {tag}: loss {loss_err:.2e} out rel-L2 {out_rel:.2e} max-abs {out_abs:.2e} worst grad {errs[wk]:.2e} "
              f"{wk} n_k {noise[wk]:.2e} zero-grad max {max(zeros.values()):.2e}")
        assert loss_err <= 5e-6, loss_err
        assert out_rel <= 2e-5 and out_abs <= 1e-3, (out_rel, out_abs)
        assert any(k.endswith("key.bias") for k in zeros)
        if L == 1:
            assert any(k.endswith("query.weight") for k in zeros) and any(k.endswith("key.weight") for k in zeros)
        else:                                # nothing else may slip under the absolute rule by a reference gone to zero
            assert all(k.endswith("key.bias") for k in zeros), sorted(zeros)
        assert bool(beta) == whole
        bad = {k: v for k, v in zeros.items() if v > 1e-6}
        assert not bad, bad
        bad = {k: v for k, v in beta.items() if v > 1e-5}
        assert not bad, bad
        bad = {k: (v, noise[k]) for k, v in errs.items() if v > max(2e-4, 4 * noise[k])}
        assert not bad, bad
    finally:
        Lb.set_default_options(**old)


@pytest.mark.parametrize("case", GENERIC, ids=_gid)
def test_generic_shape_corners_vs_float64_oracle(case):
    d, heads, L, B, c, cb, layers = case
    _check_fp32(_gid(case), d, heads, L, B, c, cb, layers, fused=0)


@pytest.mark.parametrize("no_prune_top", [0, 1])
@pytest.mark.parametrize("case", FUSED, ids=_fid)
def test_fused_cutoff_corners_vs_float64_oracle(case, no_prune_top):
    heads, L, B, c, cb, layers = case
    _check_fp32(f"{_fid(case)} fused prune={1 - no_prune_top}", 64, heads, L, B, c, cb, layers, fused=1, no_prune_top=no_prune_top)


@pytest.mark.parametrize("no_prune_top", [0, 1])
@pytest.mark.parametrize("variant", ["chain_kernels", "x3_products"])
@pytest.mark.parametrize("case", FUSED_VARIANT_CASES, ids=_fid)
def test_fused_cutoff_corners_chain_and_x3_vs_float64_oracle(case, variant, no_prune_top):
    heads, L, B, c, cb, layers = case
    _check_fp32(f"{_fid(case)} {variant} prune={1 - no_prune_top}", 64, heads, L, B, c, cb, layers, fused=1,
                no_prune_top=no_prune_top, **{variant: 1})


def test_generic_interior_shape_with_swish_vs_float64_oracle():
    _check_fp32("d100_h5_L100_B3_c21_n2 swish", 100, 5, 100, 3, 21, 11, 2, fused=0, act="swish")


@pytest.mark.parametrize("case,fused", [((64, 2, 64, 3, 15, 8, 2), 1), (GENERIC[2], 0), (GENERIC[9], 0), (GENERIC[10], 0)],
                         ids=lambda x: _gid(x) if isinstance(x, tuple) else str(x))
def test_shape_corners_bf16_vs_float64_oracle(case, fused):
    from bsarec_amd import _lib as Lb
    from test_gpu_bf16 import GRAD_GATE, LOGITS_GATE, LOSS_GATE, OUT_GATE
    d, heads, L, B, c, cb, layers = case
    ref = _reference(d, heads, L, B, c, layers, sharp=False)
    model, plan, loss = _run(ref, storage="bf16")
    assert plan.options["storage"] == 1 and plan.cfg.cutoff_bins == cb
    assert plan.lib.bsarec_plan_is_fused(plan.handle) == fused and plan.bf16 == bool(fused)
    loss_err = abs(loss - ref["loss"]) / abs(ref["loss"])
    logits = plan.view(Lb.BUF_LOGITS, 0, (B, (V + 3) // 4 * 4))[:, :V].cpu().numpy()
    lerr = float(np.abs(logits - ref["logits"]).max() / np.abs(ref["logits"]).max())
    out_err = 0.0
    for l, g, r, real in _layer_outputs(plan, ref, pruned=bool(fused)):
        out_err = max(out_err, float(np.abs(g - r)[real].max() / max(1.0, np.abs(r).max())))
    errs = {}
    for k, g in model.grad_views().items():
        g = g.cpu().numpy()
        assert np.isfinite(g).all(), k
        if k.endswith("key.bias"):
            assert np.abs(g).max() <= 1e-4, (k, np.abs(g).max())
            continue
        errs[k] = rel_l2(g, ref["G"][k])
    wk = max(errs, key=errs.get)
    print(f"shape_corners {_gid(case)} bf16: loss {loss_err:.2e} logits rel-Linf {lerr:.2e} out {out_err:.2e} worst grad "
          f"{errs[wk]:.2e} {wk}")
    assert loss_err <= LOSS_GATE and lerr <= LOGITS_GATE and out_err <= OUT_GATE, (loss_err, lerr, out_err)
    assert errs[wk] <= GRAD_GATE, {k: v for k, v in errs.items() if v > GRAD_GATE}
