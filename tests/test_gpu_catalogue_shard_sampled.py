"""Sampled-softmax head and lazy Adam inside the catalogue-sharded step (include/bsarec_shard.h, bsarec_shard_ssm_* and
bsarec_shard_lazy_*; bsarec_amd/catalogue.py with train_negatives > 0).

1. The stand-alone entry points with the W shards of one table held by ONE process (W = 2, 3, 8; ranks that own nothing;
   small catalogues so that accidental hits occur): draws, logits, loss, gradients and the owners' pull against
   tests/sampled_softmax_ref.py in float64 with the global-batch scaling; the shard's lazy mark / Adam against
   tests/lazy_adam_ref.py.
2. Two and three ranks on one GPU (gloo control plane, hipIpc mappings): three sharded steps under each sampler equal three
   steps of ONE BSARecModel with the same head on the global batch; every rank draws the candidates of the restatement.
3. The same with lazy Adam and weight decay: equal to one lazy-Adam model; rows outside the step's owned touched set keep
   w, m, v bit for bit.
4. The sampled step (dense and lazy) captured in one hipGraph over a 1-rank RCCL group replays like its eager twin, with
   fresh candidates every step; the popularity sampler without a table is refused before anything is launched.
"""
import argparse
import ctypes as C
import os
import socket

import numpy as np
import pytest

import lazy_adam_ref as LR_
import sampled_softmax_ref as R
from conftest import rel_l2

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SEED = 42
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8


def _ptrs8(L, tensors):
    return L.PTRS8(*([t.data_ptr() for t in tensors] + [None] * (8 - len(tensors))))


def _counts(V, rng):
    c = rng.integers(1, 50, size=V).astype(np.int64)
    c[rng.random(V) < 0.3] = 0
    c[0] = 0
    c[1] = max(c[1], 1)
    return c


def _state(step, t=0, lr=LR):
    """A step state (include/bsarec_hip.h): [1] = step; [3] = Adam's (step_size, bc2s) of tick t."""
    s = np.zeros(8, dtype=np.int64)
    s[1] = step
    if t:
        ss, bc = LR_.corrections(t, lr, B1, B2)
        s[3] = np.array([ss, bc], dtype=np.float32).view(np.int64)[0]
    return torch.from_numpy(s).cuda()


@pytest.mark.parametrize("sampler", ["uniform", "popularity"])
@pytest.mark.parametrize("V,W,B,N,d", [(301, 2, 24, 64, 64), (302, 3, 16, 100, 128), (5, 8, 4, 40, 64), (37, 8, 6, 70, 64)])
def test_entry_points_equal_the_restatement(V, W, B, N, d, sampler):
    from bsarec_amd import _lib as L
    lib = L.load()
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(V * 31 + W + (sampler == "popularity"))
    st = torch.cuda.current_stream().cuda_stream
    Bg, step, key = W * B, 7, (SEED * 977) & 0x7FFFFFFFFFFFFFFF
    cum = R.cumulative(_counts(V, rng)) if sampler == "popularity" else None
    cum_dev = torch.from_numpy(cum).to(dev) if cum is not None else None
    E = rng.standard_normal((V, d)) * 0.3
    rows_per = (V + W - 1) // W
    shards = []
    for r in range(W):
        t = torch.zeros(rows_per, d, device=dev)
        lo = r * rows_per
        vs = max(0, min(rows_per, V - lo))
        if vs:
            t[:vs] = torch.from_numpy(E[lo:lo + vs]).float()
        shards.append(t)
    E = np.concatenate([s.cpu().numpy() for s in shards])[:V].astype(np.float64)      # the float32 table, exactly
    # ---- draws: every rank the same stream
    state = _state(step)
    cand = torch.full((N,), -1, dtype=torch.int32, device=dev)
    corr = torch.zeros(N, device=dev)
    count = torch.full((1,), 5, dtype=torch.int32, device=dev)
    L.check(lib.bsarec_shard_ssm_draw(key, state.data_ptr(), N, V, cum_dev.data_ptr() if cum_dev is not None else None, 1,
                                      cand.data_ptr(), corr.data_ptr(), count.data_ptr(), st), "draw")
    want_c = R.draws(key, step, V, N, cum)
    np.testing.assert_array_equal(cand.cpu().numpy(), want_c)
    np.testing.assert_allclose(corr.cpu().numpy(), R.corrections(want_c, N, cum).astype(np.float32), rtol=1e-6, atol=1e-6)
    assert int(count.item()) == 0
    # ---- the global batch: h rows inside a [B, 3, d] block (row stride 3 d, as h_last sits in the layer output)
    hblk = [torch.from_numpy(rng.standard_normal((B, 3, d))).float().to(dev) for _ in range(W)]
    h_all = np.concatenate([x[:, 2, :].double().cpu().numpy() for x in hblk])
    items = np.flatnonzero(np.diff(cum, prepend=0) > 0) if cum is not None else np.arange(1, V)   # c(a) finite
    ans_all = rng.choice(items, size=Bg).astype(np.int64)
    ans_all[::3] = want_c[rng.integers(0, N, size=len(ans_all[::3]))]             # accidental hits for sure
    x_w, rows_w, loss_w, g_w = R.head(h_all, E, ans_all, want_c, cum)
    assert np.isinf(x_w).any()
    dh_w = np.einsum("bc,bcd->bd", g_w, E[np.concatenate([ans_all[:, None], np.broadcast_to(want_c, (Bg, N))], 1)])
    ans_dev = torch.from_numpy(ans_all).to(dev)
    loss_rows_all = torch.zeros(Bg, device=dev)
    grads, p8 = [], _ptrs8(L, shards)
    for r in range(W):
        sl = slice(r * B, (r + 1) * B)
        ans_r = ans_dev[sl].contiguous()
        rows = torch.full((B + N, d), 7.0, device=dev)
        L.check(lib.bsarec_shard_ssm_gather(ans_r.data_ptr(), B, cand.data_ptr(), N, C.byref(p8), W, rows_per, V, d, rows.data_ptr(),
                                            st), "gather")
        np.testing.assert_array_equal(rows.cpu().numpy(), np.concatenate([E[ans_all[sl]], E[want_c]]).astype(np.float32))
        h, ldh = hblk[r].data_ptr() + 4 * 2 * d, 3 * d
        logits = torch.zeros(B, N + 1, device=dev)
        dlogits = torch.zeros(B, N + 1, device=dev)
        lrows = torch.zeros(B, device=dev)
        L.check(lib.bsarec_shard_ssm_head(h, ldh, B, Bg, rows.data_ptr(), ans_r.data_ptr(), cand.data_ptr(), corr.data_ptr(), N, V,
                                          cum_dev.data_ptr() if cum_dev is not None else None, 1, d, logits.data_ptr(),
                                          dlogits.data_ptr(), lrows.data_ptr(), st), "head")
        np.testing.assert_allclose(logits.double().cpu().numpy(), x_w[sl], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(lrows.double().cpu().numpy(), rows_w[sl], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(dlogits.double().cpu().numpy(), g_w[sl], rtol=1e-4, atol=2e-6 / Bg)   # fp32 lse: ~1 ulp
        loss_rows_all[sl] = lrows
        dout = torch.full((B, 3, d), 5.0, device=dev)
        grad = torch.full((B + N, d), 9.0, device=dev)
        scratch = torch.zeros(lib.bsarec_shard_ssm_bwd_scratch_floats(B, N, d), device=dev)
        L.check(lib.bsarec_shard_ssm_bwd(dlogits.data_ptr(), B, N, h, ldh, rows.data_ptr(), d, dout.data_ptr() + 4 * 2 * d, 3 * d,
                                         grad.data_ptr(), scratch.data_ptr(), st), "bwd")
        np.testing.assert_allclose(dout[:, 2].double().cpu().numpy(), dh_w[sl], rtol=1e-4, atol=1e-6)
        assert float((dout[:, :2] - 5.0).abs().max()) == 0.0                 # only position L-1 written
        gd = grad.double().cpu().numpy()
        np.testing.assert_allclose(gd[:B], g_w[sl, :1] * h_all[sl], rtol=1e-4, atol=1e-5 / Bg)
        np.testing.assert_allclose(gd[B:], g_w[sl, 1:].T @ h_all[sl], rtol=1e-4, atol=1e-5 / Bg)
        grads.append(grad)
    loss = torch.zeros(1, device=dev)
    L.check(lib.bsarec_shard_ssm_loss(loss_rows_all.data_ptr(), Bg, loss.data_ptr(), st), "loss")
    assert abs(float(loss.item()) - loss_w) <= 1e-5 * max(1.0, abs(loss_w))
    # ---- owners' pull: dE of the head = sum over all columns of g_bc h_b
    cols = np.concatenate([ans_all[:, None], np.broadcast_to(want_c, (Bg, N))], 1)
    dE_w = np.zeros((V, d))
    np.add.at(dE_w, cols.reshape(-1), (g_w[:, :, None] * h_all[:, None, :]).reshape(-1, d))
    g8 = _ptrs8(L, grads)
    for r in range(W):
        lo = r * rows_per
        vs = max(0, min(rows_per, V - lo))
        dE = torch.zeros(rows_per, d, device=dev)
        L.check(lib.bsarec_shard_ssm_pull(ans_dev.data_ptr(), B, W, cand.data_ptr(), N, C.byref(g8), lo, vs, V, d, dE.data_ptr(), st),
                "pull")
        if vs:
            np.testing.assert_allclose(dE[:vs].double().cpu().numpy(), dE_w[lo:lo + vs], rtol=1e-4, atol=1e-5 / Bg)
        if rows_per > vs:
            assert float(dE[vs:].abs().max()) == 0.0
    # ---- lazy Adam of the shards: mark T_own, update it, nothing else
    n = 30
    ids_all = rng.integers(0, V, size=(W, n)).astype(np.int64)
    ids_all[:, ::4] = 0
    ids_dev = torch.from_numpy(ids_all).to(dev)
    T = LR_.touched(ids_all, ans_all, want_c, V)
    t, wd = 3, 0.01
    for r in range(W):
        lo = r * rows_per
        vs = max(0, min(rows_per, V - lo))
        cap = min(vs, W * n + Bg + N)
        mark = torch.zeros(max(vs, 1), dtype=torch.int32, device=dev)
        rows = torch.zeros(max(cap, 1), dtype=torch.int32, device=dev)
        cnt = torch.zeros(1, dtype=torch.int32, device=dev)
        L.check(lib.bsarec_shard_lazy_mark(ids_dev.data_ptr(), W * n, ans_dev.data_ptr(), Bg, cand.data_ptr(), N, lo, vs, V,
                                           mark.data_ptr(), rows.data_ptr(), cnt.data_ptr(), cap, st), "mark")
        own = T[(T >= lo) & (T < lo + vs)] - lo
        k = int(cnt.item())
        assert k == len(own)
        np.testing.assert_array_equal(np.sort(rows[:k].cpu().numpy()), own)
        w0, m0, v0 = (rng.standard_normal((rows_per, d)).astype(np.float32) for _ in range(3))
        v0 = np.abs(v0)
        g0 = rng.standard_normal((rows_per, d)).astype(np.float32)
        w, m, v, g = (torch.from_numpy(x.copy()).to(dev) for x in (w0, m0, v0, g0))
        L.check(lib.bsarec_shard_lazy_adam(w.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), d, B1, B2, EPS, wd, mark.data_ptr(),
                                           rows.data_ptr(), cnt.data_ptr(), cap, _state(step, t).data_ptr(), st), "lazy_adam")
        ww, mw, vw = LR_.lazy_step(w0, m0, v0, g0[own], own, t, LR, B1, B2, EPS, wd)
        out = np.setdiff1d(np.arange(rows_per), own)
        for now, want, before in ((w, ww, w0), (m, mw, m0), (v, vw, v0)):
            now = now.cpu().numpy()
            np.testing.assert_array_equal(now[out], before[out])             # untouched rows: bit for bit, no weight decay
            if len(own):
                assert rel_l2(now[own], want[own]) <= 1e-6
        gw = g0.copy()
        gw[own] = 0
        np.testing.assert_array_equal(g.cpu().numpy(), gw)                     # T_own's gradient rows zeroed, others kept
        assert int(mark.sum().item()) == 0                                    # marks cleared


# ---- ranks ------------------------------------------------------------------------------------------------------------
def _ns(**kw):
    a = argparse.Namespace(item_size=301, hidden_size=64, max_seq_length=50, batch_size=32, hidden_dropout_prob=0.0,
                           attention_probs_dropout_prob=0.0, num_hidden_layers=2, num_attention_heads=2,
                           hidden_act="gelu", initializer_range=0.02, c=3, alpha=0.9, seed=SEED, lr=LR,
                           adam_beta1=B1, adam_beta2=B2, weight_decay=0.0, no_cuda=False, log_freq=1, train_negatives=64)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


HEADS = {"uniform": dict(train_sampler="uniform"), "popularity": dict(train_sampler="popularity"),
         "popularity_nologq": dict(train_sampler="popularity", train_no_logq=True)}


def _batches(ns, steps, Bg):
    g = torch.Generator(device="cpu").manual_seed(5)
    V, Lq = ns.item_size, ns.max_seq_length
    out = []
    for _ in range(steps):
        ids = torch.randint(1, V, (Bg, Lq), generator=g)
        pad = torch.randint(0, Lq - 2, (Bg,), generator=g)
        ids[torch.arange(Lq)[None, :] < pad[:, None]] = 0
        out.append((ids, torch.randint(1, V, (Bg,), generator=g)))
    return out


def _pop(ns):
    """Popularity counts with every real item drawable (an answer of count 0 would have c(a) = -inf)."""
    c = np.random.default_rng(ns.item_size).integers(1, 50, size=ns.item_size).astype(np.int64)
    c[0] = 0
    return c


def _full_model(ns):
    from bsarec_amd import BSARecModel
    torch.manual_seed(3)
    return BSARecModel(ns).cuda()


def _worker(rank, world, port, kw, heads, out_dir):
    import torch.distributed as dist
    from bsarec_amd.catalogue import ShardedCatalogue
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        for name in heads:
            ns = _ns(**kw, **HEADS[name])
            B = ns.batch_size
            init = _full_model(ns).state_dict()
            sc = ShardedCatalogue(ns, B, dist.group.WORLD, "cuda:0")
            sc.load_full_state_dict(init)
            if ns.train_sampler == "popularity":
                sc.set_train_popularity(_pop(ns))
            losses, cands, snap = [], [], {}
            for s, (ids, ans) in enumerate(_batches(ns, 3, world * B)):
                if s == 2:
                    torch.cuda.synchronize()
                    snap = {"pre_E": sc.E.cpu().numpy().copy(), "pre_m": sc.m.cpu().numpy().copy(), "pre_v": sc.v.cpu().numpy().copy()}
                losses.append(float(sc.train_step(ids[rank * B:(rank + 1) * B], ans[rank * B:(rank + 1) * B])))
                cands.append(sc.cand.cpu().numpy().copy())
            snap.update(post_E=sc.E.cpu().numpy(), post_m=sc.m.cpu().numpy(), post_v=sc.v.cpu().numpy())
            assert not sc.px.timed_out()
            sd = {k: v.detach().cpu().numpy() for k, v in sc.full_state_dict().items()}
            np.savez(os.path.join(out_dir, f"{name}_rank{rank}.npz"), losses=np.asarray(losses), cands=np.stack(cands),
                     lo=sc.lo, Vs=sc.Vs, **{"snap/" + k: v for k, v in snap.items()}, **sd)
            sc.close()
    finally:
        dist.destroy_process_group()


def _spawn(fn, world, *args):
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(fn, args=(world, port) + args, nprocs=world, join=True)


CASES = [(2, dict()), (2, dict(hidden_size=128, max_seq_length=64, num_attention_heads=4, item_size=1003, c=9)),
         (3, dict(item_size=302, batch_size=16))]
CASE_IDS = ["W2_fused_d64_L50", "W2_generic_d128_L64", "W3_uneven_shards"]


def _check_against_one_model(world, kw, heads, lazy, tmp_path):
    for name in heads:
        ns = _ns(**kw, **HEADS[name])
        if lazy:
            ns.train_lazy_adam = True
        r0 = np.load(tmp_path / f"{name}_rank0.npz")
        keys = [k for k in r0.files if k not in ("losses", "cands", "lo", "Vs") and not k.startswith("snap/")]
        cum = R.cumulative(_pop(ns)) if ns.train_sampler == "popularity" else None
        for r in range(world):
            rr = np.load(tmp_path / f"{name}_rank{r}.npz")
            for s in range(3):                                            # the draws of ONE model with the same seed
                np.testing.assert_array_equal(rr["cands"][s], R.draws(SEED, s + 1, ns.item_size, ns.train_negatives, cum))
            for k in keys + ["losses"]:
                np.testing.assert_array_equal(r0[k], rr[k], err_msg=k)   # replicas bit-identical, same loss on every rank
        model = _full_model(ns)
        if cum is not None:
            model.set_train_popularity(_pop(ns))
        model.configure_adam(lr=ns.lr, betas=(ns.adam_beta1, ns.adam_beta2), weight_decay=ns.weight_decay)
        model.train()
        losses, g3 = [], None
        for s, (ids, ans) in enumerate(_batches(ns, 3, world * ns.batch_size)):
            losses.append(float(model.train_step(ids.cuda(), ans.cuda())))
            if s == 2 and lazy:
                g3 = model.grad_views()["item_embeddings.weight"].detach().cpu().numpy().copy()
        np.testing.assert_allclose(r0["losses"], losses, atol=2e-4, err_msg=name)
        sd = model.state_dict()
        assert set(sd) == set(keys)
        for k in sd:
            if lazy and k.endswith("key.bias"):
                continue        # d loss / d key.bias is 0 in exact arithmetic: with weight decay, Adam follows its rounding noise
            got, want = r0[k], sd[k].detach().cpu().numpy()
            assert got.shape == want.shape, k
            bad = np.abs(got - want) > 2e-5
            assert bad.mean() <= 2e-3, (name, k, bad.mean(), np.abs(got - want).max())
        if not lazy:
            continue
        # across the third step: outside T_own every shard row keeps w, m, v bit for bit; T_own's rows are the lazy update
        # of their own pre-step state with the step's gradient (the one model's rows of T hold it after its lazy step)
        ids, ans = _batches(ns, 3, world * ns.batch_size)[2]
        T = LR_.touched(ids.numpy(), ans.numpy(), r0["cands"][2], ns.item_size)
        for r in range(world):
            rr = np.load(tmp_path / f"{name}_rank{r}.npz")
            lo, vs = int(rr["lo"]), int(rr["Vs"])
            own = T[(T >= lo) & (T < lo + vs)] - lo
            out = np.setdiff1d(np.arange(len(rr["snap/pre_E"])), own)
            for q in ("E", "m", "v"):
                np.testing.assert_array_equal(rr[f"snap/post_{q}"][out], rr[f"snap/pre_{q}"][out], err_msg=q)
            assert len(own) > 0
            w, m, v = LR_.lazy_step(rr["snap/pre_E"], rr["snap/pre_m"], rr["snap/pre_v"], g3[own + lo], own, 3, ns.lr, B1, B2, EPS,
                                    ns.weight_decay)
            for q, want in (("E", w), ("m", m), ("v", v)):
                got = rr[f"snap/post_{q}"][own]
                bad = np.abs(got - want[own]) > 2e-5
                assert bad.mean() <= 2e-3, (q, bad.mean(), np.abs(got - want[own]).max())
                assert not np.array_equal(got, rr[f"snap/pre_{q}"][own]), q


@pytest.mark.parametrize("world,kw", CASES, ids=CASE_IDS)
def test_ranks_sampled_head_equals_one_model_on_the_global_batch(world, kw, tmp_path):
    heads = list(HEADS)
    _spawn(_worker, world, kw, heads, str(tmp_path))
    _check_against_one_model(world, kw, heads, False, tmp_path)


@pytest.mark.parametrize("world,kw", CASES, ids=CASE_IDS)
def test_ranks_lazy_adam_equals_one_lazy_model(world, kw, tmp_path):
    heads = ["uniform", "popularity"]
    kw = dict(kw, train_lazy_adam=True, weight_decay=0.01)
    _spawn(_worker, world, kw, heads, str(tmp_path))
    _check_against_one_model(world, kw, heads, True, tmp_path)


# ---- graph ------------------------------------------------------------------------------------------------------------
def _graph_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    from bsarec_amd.catalogue import ShardedCatalogue
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                            device_id=torch.device("cuda", 0))
    try:
        res = {}
        for lazy in (False, True):
            ns = _ns(hidden_dropout_prob=0.3, attention_probs_dropout_prob=0.2, train_sampler="popularity",
                     train_lazy_adam=lazy, weight_decay=0.01 if lazy else 0.0)
            B = ns.batch_size
            for mode in ("eager", "graph"):
                torch.manual_seed(7)
                sc = ShardedCatalogue(ns, B, dist.group.WORLD, "cuda:0")
                if not lazy and mode == "eager":               # refused on the host before anything is launched
                    ids, ans = _batches(ns, 1, B)[0]
                    with pytest.raises(ValueError, match="set_train_popularity"):
                        sc.train_step(ids.cuda(), ans.cuda())
                    torch.cuda.synchronize()
                    assert int(sc.encoder._state[1].item()) == 0
                sc.set_train_popularity(_pop(ns))
                losses, cands = [], []
                for ids, ans in _batches(ns, 4, B):
                    step = sc.train_step_graph if mode == "graph" else sc.train_step
                    losses.append(float(step(ids.cuda(), ans.cuda()).item()))
                    cands.append(sc.cand.cpu().numpy().copy())
                if mode == "graph":
                    assert sc.graph_captured, getattr(sc, "_graph_error", "no capture attempted")
                sc.check_exchange()
                tag = f"{'lazy' if lazy else 'dense'}_{mode}"
                res[tag] = (losses, cands, {k: v.detach().cpu().numpy() for k, v in sc.full_state_dict().items()})
                sc.close()
        out = {}
        for tag, (losses, cands, sd) in res.items():
            out[tag + "/losses"], out[tag + "/cands"] = np.asarray(losses), np.stack(cands)
            out.update({f"{tag}/sd/{k}": v for k, v in sd.items()})
        np.savez(os.path.join(out_dir, "graph.npz"), **out)
    finally:
        dist.destroy_process_group()


def test_sampled_sharded_step_replays_from_one_graph_rccl_one_rank(tmp_path):
    _spawn(_graph_worker, 1, str(tmp_path))
    z = np.load(tmp_path / "graph.npz")
    for kind in ("dense", "lazy"):
        e, g = f"{kind}_eager", f"{kind}_graph"
        np.testing.assert_allclose(z[g + "/losses"], z[e + "/losses"], rtol=1e-5)
        np.testing.assert_array_equal(z[g + "/cands"], z[e + "/cands"])
        c = z[g + "/cands"]
        assert all(not np.array_equal(c[i], c[i + 1]) for i in range(len(c) - 1))   # fresh candidates every replay
        for k in [k[len(e) + 4:] for k in z.files if k.startswith(e + "/sd/")]:
            if kind == "lazy" and k.endswith("key.bias"):
                continue        # (weight decay on a parameter whose gradient is 0 in exact arithmetic: see above)
            a, b = z[f"{g}/sd/{k}"], z[f"{e}/sd/{k}"]
            bad = np.abs(a - b) > 2e-5
            assert bad.mean() <= 2e-3, (kind, k, bad.mean(), np.abs(a - b).max())
