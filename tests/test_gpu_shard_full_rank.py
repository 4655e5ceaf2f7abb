"""bsarec_topk_full_range (full ranking over a contiguous item range: global seen ids in, global ids out) and the fused
evaluation of ShardedCatalogue.

1. The entry point alone: the col_base = 0 case against bsarec_topk_full; the partition property (the merge of the ranges' lists
   under the total order IS the whole table's list, bit for bit -- a score depends on the h row and the item row only);
   integer data against bsarec_topk_seen on the materialised slice; graph capture; one shard of C5 at its own shape.
2. Two and three ranks on one GPU (gloo control plane, hipIpc mappings): ShardedCatalogue.topk(full_rank="fused") against
   bsarec_topk_full on the gathered table (exact), against the dense sharded path (its own gates), the metrics, and the memory
   of an evaluation under the sampled-softmax head.
"""
import os
import socket

import numpy as np
import pytest

import full_rank_ref as R

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _lib():
    from bsarec_amd import _lib
    return _lib, _lib.load()


def csr_of(seen):
    indptr = np.zeros(len(seen) + 1, np.int64)
    indptr[1:] = np.cumsum([len(s) for s in seen])
    indices = np.array([i for s in seen for i in s], np.int64)
    return torch.from_numpy(indptr).cuda(), torch.from_numpy(indices if len(indices) else np.zeros(1, np.int64)).cuda()


def _call(name, h, E, base, seen, k, cap):
    L, lib = _lib()
    B, d = h.shape
    V = E.shape[0]
    nb = lib.bsarec_topk_full_workspace_bytes(B, V, d, k, cap)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    idx = torch.full((B, k), -7, dtype=torch.int64, device="cuda")
    val = torch.full((B, k), -7.0, dtype=torch.float32, device="cuda")
    ptrs = (None, None, None)
    if seen is not None:
        indptr, indices = csr_of(seen)
        users = torch.arange(B, device="cuda")
        ptrs = (users.data_ptr(), indptr.data_ptr(), indices.data_ptr())
    st = torch.cuda.current_stream().cuda_stream
    tail = (*ptrs, k, cap, ws.data_ptr(), nb, idx.data_ptr(), val.data_ptr(), st)
    if name == "range":
        L.check(lib.bsarec_topk_full_range(h.data_ptr(), h.stride(0), E.data_ptr(), B, V, base, d, *tail), "bsarec_topk_full_range")
    else:
        L.check(lib.bsarec_topk_full(h.data_ptr(), h.stride(0), E.data_ptr(), B, V, d, *tail), "bsarec_topk_full")
    torch.cuda.synchronize()
    return idx.cpu().numpy(), val.cpu().numpy()


def ranged(h, E, base, seen, k, cap=0):
    """bsarec_topk_full_range over the rows E (device, contiguous: rows [base, base + len(E)) of a catalogue); seen: GLOBAL ids."""
    return _call("range", h, E, base, seen, k, cap)


def whole(h, E, seen, k, cap=0):
    return _call("full", h, E, 0, seen, k, cap)


def dense(S, seen, k):
    """bsarec_topk_seen on the fp32 matrix S [B, V] (device); seen: local ids."""
    L, lib = _lib()
    S = S.clone()
    B, V = S.shape
    idx = torch.empty(B, k, dtype=torch.int64, device="cuda")
    val = torch.empty(B, k, dtype=torch.float32, device="cuda")
    ptrs = (None, None, None)
    if seen is not None:
        indptr, indices = csr_of(seen)
        users = torch.arange(B, device="cuda")
        ptrs = (users.data_ptr(), indptr.data_ptr(), indices.data_ptr())
    L.check(lib.bsarec_topk_seen(S.data_ptr(), S.stride(0), B, V, *ptrs, k, idx.data_ptr(), val.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream), "bsarec_topk_seen")
    torch.cuda.synchronize()
    return idx.cpu().numpy(), val.cpu().numpy()


def assert_same(gi, gv, wi, wv, msg=""):
    np.testing.assert_array_equal(gi, wi, err_msg=msg)
    np.testing.assert_array_equal(gv.view(np.uint32), wv.view(np.uint32), err_msg=msg)


def merge(ids, vals, k):
    """Host merge of concatenated candidate lists under the total order: NaN first, then descending with -0 = +0, then the
    smaller global id (tests/full_rank_ref.py's keys)."""
    out_i, out_v = np.empty((ids.shape[0], k), np.int64), np.empty((ids.shape[0], k), np.float32)
    for b in range(ids.shape[0]):
        order = np.lexsort((ids[b], R.order_keys(vals[b]), ~np.isnan(vals[b])))[:k]
        out_i[b], out_v[b] = ids[b][order], vals[b][order]
    return out_i, out_v


def float_case(B, V, d, seed, scale=0.3):
    rng = np.random.default_rng(seed)
    h = torch.from_numpy(rng.standard_normal((B, d)).astype(np.float32)).cuda()
    E = torch.from_numpy((rng.standard_normal((V, d)) * scale).astype(np.float32)).cuda()
    return rng, h, E


@pytest.mark.parametrize("k", [1, 20, 100, 1024])
def test_base_zero_over_the_whole_table_is_topk_full(k):
    B, V, d = 40, 20_011, 64
    rng, h, E = float_case(B, V, d, seed=k)
    seen = [rng.choice(V, size=int(rng.integers(0, 80)), replace=False).tolist() + [-1, V + 3] for _ in range(B)]
    wi, wv = whole(h, E, seen, k)
    gi, gv = ranged(h, E, 0, seen, k)
    assert_same(gi, gv, wi, wv)
    gi, gv = ranged(h, E, 0, None, k)
    assert_same(gi, gv, *whole(h, E, None, k))
    assert gi.min() >= 0 and gi.max() < V


def global_seen(rng, B, V, k, best):
    """Per row: ids inside every range, ids outside the catalogue, -1 pads, duplicates; rows b % 3 == 0 have seen their best
    items; row 1 holds more than 2,048 entries (more than one chunk of the select kernel's LDS hash)."""
    seen = []
    for b in range(B):
        s = rng.integers(0, V, size=int(rng.integers(0, 3 * k + 5))).tolist()
        s += s[: len(s) // 3]                                # duplicates
        if b % 3 == 0:
            s += best[b].tolist()
        s += [-1, -1, V, V + 11, 2 * V + 1, -5]
        if b == 1:
            s += rng.integers(0, V, size=2500).tolist() + best[b].tolist()
        rng.shuffle(s)
        seen.append([int(x) for x in s])
    assert len(seen[1]) > 2048
    return seen


@pytest.mark.parametrize("W", [2, 3, 8])
@pytest.mark.parametrize("V", [40, 3417, 100_003])
def test_partition_merge_is_the_whole_tables_list_on_float_data(V, W):
    """Contiguous ranges of ceil(V / W) rows (an uneven, at V = 40 / W = 8 a short, last range; ranges shorter than k give their
    min(k, Vs) best): the host merge under the total order equals bsarec_topk_full on the whole table, ids and values bit for
    bit -- no tolerance: a score does not depend on the item's position."""
    B, d, k = 33, 64, 20
    rng, h, E = float_case(B, V, d, seed=V + W)
    best = torch.topk(h @ E.T, min(V, k + 2), dim=1).indices.cpu().numpy()
    seen = global_seen(rng, B, V, k, best)
    wi, wv = whole(h, E, seen, k)
    rows_per = (V + W - 1) // W
    parts_i, parts_v = [], []
    for r in range(W):
        lo = r * rows_per
        vs = max(0, min(rows_per, V - lo))
        if vs == 0:
            continue
        kk = min(k, vs)
        gi, gv = ranged(h, E[lo:lo + vs], lo, seen, kk)
        assert gi.min() >= lo and gi.max() < lo + vs
        parts_i.append(gi)
        parts_v.append(gv)
    assert len(parts_i) >= 2
    mi, mv = merge(np.concatenate(parts_i, 1), np.concatenate(parts_v, 1), k)
    assert_same(mi, mv, wi, wv)


def int_slice(B, Vs, d, seed, base, k=20, lo=-3, hi=3):
    """Integer h and item rows (every partial sum an integer below 2^24: every summation order gives the same fp32 score, and
    ties are massive), S = h E^T in fp64 on the device, and seen lists: local ones for the dense path and the same items as
    global ids mixed with other ranges' ids, pads and duplicates for the range call."""
    rng = np.random.default_rng(seed)
    h = rng.integers(lo, hi + 1, size=(B, d)).astype(np.float32)
    E = rng.integers(-3, 4, size=(Vs, d)).astype(np.float32)
    S = (torch.from_numpy(h).cuda().double() @ torch.from_numpy(E).cuda().double().T).float()
    best = torch.topk(S, min(Vs, k + 2), dim=1).indices.cpu().numpy()
    local, glob = [], []
    for b in range(B):
        s = rng.choice(Vs, size=int(rng.integers(0, min(Vs, 3 * k + 5))), replace=False).tolist()
        if b % 3 == 0:
            s += best[b].tolist()
        g = [x + base for x in s] + [x + base for x in s[:5]]
        g += [-1, -1, base + Vs, base + Vs + 5] + ([base - 1, int(rng.integers(0, base))] if base else [])
        rng.shuffle(g)
        local.append([int(x) for x in s])
        glob.append([int(x) for x in g])
    return h, E, S, local, glob


def check_against_dense(h, E, S, local, glob, base, k, caps=(0,)):
    if not torch.is_tensor(S):
        S = torch.from_numpy(S).cuda()
    ht, Et = torch.from_numpy(h).cuda(), torch.from_numpy(E).cuda()
    di, dv = dense(S, local, k)
    for cap in caps:
        gi, gv = ranged(ht, Et, base, glob, k, cap)
        assert_same(gi, gv, di + base, dv, msg=f"cap {cap}")


@pytest.mark.parametrize("B,Vs,d,k,base", [(3, 1000, 64, 20, 7_000_001), (257, 4097, 16, 100, 4097), (33, 100_003, 64, 20, 300_009),
                                           (4, 4097, 64, 1024, 2**31 - 1 - 4097), (1, 20, 16, 20, 20), (64, 5000, 256, 20, 0)])
def test_bit_exact_against_topk_seen_on_the_slice_integer_data(B, Vs, d, k, base):
    """Also with cand_cap = k and an odd capacity (the re-threshold rounds and the fallback kernel)."""
    h, E, S, local, glob = int_slice(B, Vs, d, seed=B + Vs + k, base=base, k=k)
    odd = k + 37 if (k + 37) % 2 else k + 38
    check_against_dense(h, E, S, local, glob, base, k, caps=(0, k, odd))
    check_against_dense(h, E, S, None, None, base, k, caps=(0, k))


def test_negative_rows_nan_row_and_all_zero_table():
    base, B, Vs, d, k = 1_250_001, 64, 5000, 64, 20
    h, E, S, local, glob = int_slice(B, Vs, d, seed=5, base=base, k=k)
    h = -np.abs(h) - 1
    E = np.abs(E) + 1                                   # every score < 0: the seen zeros come first (the fallback kernel's rows)
    S = (h.astype(np.float64) @ E.astype(np.float64).T).astype(np.float32)
    check_against_dense(h, E, S, local, glob, base, k, caps=(0, k, 41))
    check_against_dense(h, E, S, None, None, base, k, caps=(0, k))
    # a NaN row: every score NaN -> the first k items of the range, except that its seen items are 0 and rank below
    h2, E2, S2, local2, glob2 = int_slice(8, 3000, d, seed=6, base=base, k=k)
    h2[3, :] = np.nan
    S2 = np.full((8, 3000), np.nan, np.float32)
    with np.errstate(invalid="ignore"):
        S2[:] = (h2.astype(np.float64) @ E2.astype(np.float64).T).astype(np.float32)
    check_against_dense(h2, E2, S2, local2, glob2, base, k, caps=(0, k))
    gi, gv = ranged(torch.from_numpy(h2).cuda(), torch.from_numpy(E2).cuda(), base, None, k)
    assert (gi[3] == base + np.arange(k)).all() and np.isnan(gv[3]).all()
    # an all-zero table: everything ties, the list is the range's first k ids
    Z = np.zeros((Vs, d), np.float32)
    SZ = np.zeros((B, Vs), np.float32)
    check_against_dense(h, Z, SZ, local, glob, base, k, caps=(0, k))
    gi, gv = ranged(torch.from_numpy(h).cuda(), torch.from_numpy(Z).cuda(), base, glob, 100)
    assert (gi == base + np.arange(100)).all() and (gv == 0).all()


def test_graph_capture_replays_the_eager_lists():
    L, lib = _lib()
    B, V, d, k, base = 64, 50_000, 64, 20, 150_000
    rng, h, E = float_case(B, V, d, seed=6, scale=1.0)
    seen = [(base + rng.choice(V, size=30, replace=False)).tolist() + [-1, 5, base + V] for _ in range(B)]
    indptr, indices = csr_of(seen)
    users = torch.arange(B, device="cuda")
    nb = lib.bsarec_topk_full_workspace_bytes(B, V, d, k, 0)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    idx = torch.empty(B, k, dtype=torch.int64, device="cuda")
    val = torch.empty(B, k, dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()

    def call(stream):
        L.check(lib.bsarec_topk_full_range(h.data_ptr(), d, E.data_ptr(), B, V, base, d, users.data_ptr(), indptr.data_ptr(),
                                           indices.data_ptr(), k, 0, ws.data_ptr(), nb, idx.data_ptr(), val.data_ptr(),
                                           stream.cuda_stream), "bsarec_topk_full_range")
    with torch.cuda.stream(s):
        call(s)                                          # eager warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.cuda.stream(s):
        call(s)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() == before   # no allocation
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(s)
    torch.cuda.synchronize()
    h.copy_(torch.from_numpy(rng.standard_normal((B, d)).astype(np.float32)))
    E.copy_(torch.from_numpy(rng.standard_normal((V, d)).astype(np.float32)))
    g.replay()
    torch.cuda.synchronize()
    gi, gv = idx.cpu().numpy(), val.cpu().numpy()
    ei, ev = ranged(h, E, base, seen, k)
    assert_same(gi, gv, ei, ev)
    assert gi.min() >= base and gi.max() < base + V


def test_one_shard_of_C5_at_its_own_shape():
    """BASELINE.json C5 sharded 8 ways: rank 3's evaluation at ITS shape -- 1,250,001 owned rows, d = 256, the node's 8 x 256
    sequences, k = 20, column base 3 x 1,250,001.  Integer data (entries in -3 .. 3: |score| <= 2,304, every sum exact); 50
    global seen ids per row, half of them inside the range.  32 sampled rows against a chunked torch restatement: scores in
    float64, seen := 0, a stable descending sort (ties to the smaller id)."""
    Vs, d, Bg, k = 1_250_001, 256, 2048, 20
    base = 3 * Vs
    dev = torch.device("cuda:0")
    g = torch.Generator(device="cuda").manual_seed(1)
    E = torch.randint(-3, 4, (Vs, d), device=dev, generator=g).float()
    h = torch.randint(-3, 4, (Bg, d), device=dev, generator=g).float()
    rows = torch.randperm(Bg, device=dev, generator=g)[:32].sort().values
    scores = torch.empty(32, Vs, dtype=torch.float64, device=dev)
    for c in range(0, Vs, 131072):
        scores[:, c:c + 131072] = h[rows].double() @ E[c:c + 131072].double().T
    inside = base + torch.randint(0, Vs, (Bg, 25), device=dev, generator=g)
    inside[rows[::2], :5] = torch.topk(scores[::2], 5, dim=1).indices + base       # half of the sampled rows have seen their 5 best
    outside = torch.randint(0, 8 * Vs, (Bg, 25), device=dev, generator=g)
    outside = torch.where((outside >= base) & (outside < base + Vs), outside - base, outside)      # other ranks' items
    seen_t = torch.cat([inside, outside], 1)[:, torch.randperm(50, device=dev, generator=g)].contiguous()
    L, lib = _lib()
    nb = lib.bsarec_topk_full_workspace_bytes(Bg, Vs, d, k, 0)
    assert 0 < nb < 512 << 20                            # the score matrix: 10.2 GB
    ws = torch.empty(nb, dtype=torch.uint8, device=dev)
    idx = torch.empty(Bg, k, dtype=torch.int64, device=dev)
    val = torch.empty(Bg, k, dtype=torch.float32, device=dev)
    users = torch.arange(Bg, device=dev)
    indptr = torch.arange(Bg + 1, device=dev) * 50
    L.check(lib.bsarec_topk_full_range(h.data_ptr(), d, E.data_ptr(), Bg, Vs, base, d, users.data_ptr(), indptr.data_ptr(),
                                       seen_t.data_ptr(), k, 0, ws.data_ptr(), nb, idx.data_ptr(), val.data_ptr(),
                                       torch.cuda.current_stream().cuda_stream), "bsarec_topk_full_range")
    torch.cuda.synchronize()
    assert int(idx.min()) >= base and int(idx.max()) < base + Vs
    loc = seen_t[rows] - base
    ok = (loc >= 0) & (loc < Vs)
    r32 = torch.arange(32, device=dev).view(32, 1).expand(32, 50)
    scores[r32[ok], loc[ok]] = 0.0
    sv, si = torch.sort(scores, dim=1, descending=True, stable=True)
    want_i, want_v = (si[:, :k] + base).cpu().numpy(), sv[:, :k].float().cpu().numpy()
    assert_same(idx[rows].cpu().numpy(), val[rows].cpu().numpy(), want_i, want_v)


# ---- ranks -------------------------------------------------------------------------------------------------------------
def _eval_worker(rank, world, port, kw, out_dir):
    import torch.distributed as dist
    from bsarec_amd.catalogue import ShardedCatalogue
    from test_gpu_catalogue_shard import _batches, _full_model, _ns, _seen
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        ns = _ns(**kw)
        B = ns.batch_size
        sc = ShardedCatalogue(ns, B, dist.group.WORLD, "cuda:0")
        sc.load_full_state_dict(_full_model(ns).state_dict())
        for ids, ans in _batches(ns, 3, world * B):
            sc.train_step(ids[rank * B:(rank + 1) * B], ans[rank * B:(rank + 1) * B])
        assert not sc.px.timed_out()
        ids, _ = _batches(ns, 1, world * B)[0]
        seen = _seen(ns, world * B)
        mine = slice(rank * B, (rank + 1) * B)
        fv, fi = sc.topk(ids[mine], 20, seen[mine], full_rank="fused")
        torch.cuda.synchronize()
        h_all = sc.h_all.cpu().numpy().copy()
        dv, di = sc.topk(ids[mine], 20, seen[mine])                    # the dense path: the default
        nv, ni = sc.topk(ids[mine], 20, None, full_rank="fused")       # no seen lists
        # the metrics through the fused path: every rank must report the GLOBAL numbers
        ans_hit = fi[:, 2].clone()
        vals, txt = sc.full_sort_scores([(ids[mine], ans_hit, seen[mine])], epoch=3, full_rank="fused")
        assert vals[0] == 1.0 and vals[2] == 1.0 and vals[4] == 1.0 and abs(vals[1] - 0.5) < 1e-12 and abs(vals[5] - 0.5) < 1e-12, vals
        assert txt.startswith("{'Epoch': 3, 'HR@5': '1.0000', 'NDCG@5': '0.5000'")
        ans_mixed = torch.where(torch.arange(B, device=fi.device) % 2 == 0, fi[:, 0], fi[:, 19])
        if rank % 2 == 1:
            ans_mixed = fi[:, 7]
        sc.args.eval_full_rank = "fused"                                # the flag the single-GPU Trainer honours
        vals2, _ = sc.full_sort_scores([(ids[mine], ans_mixed, seen[mine])])
        sd = {k: v.detach().cpu().numpy() for k, v in sc.full_state_dict().items()}
        np.savez(os.path.join(out_dir, f"eval{rank}.npz"), fv=fv.cpu().numpy(), fi=fi.cpu().numpy(), dv=dv.cpu().numpy(),
                 di=di.cpu().numpy(), nv=nv.cpu().numpy(), ni=ni.cpu().numpy(), h_all=h_all, vals2=np.asarray(vals2),
                 ans_mixed=ans_mixed.cpu().numpy(), E=sd["item_embeddings.weight"])
        sc.close()
    finally:
        dist.destroy_process_group()


def _spawn(fn, world, *args):
    import torch.multiprocessing as mp
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(fn, args=(world, port) + args, nprocs=world, join=True)


@pytest.mark.parametrize("world,kw", [(2, dict()), (3, dict(item_size=302, batch_size=16))], ids=["W2", "W3_uneven_shards"])
def test_ranks_fused_topk_equals_topk_full_on_the_gathered_table(world, kw, tmp_path):
    """(W3: 302 rows over 3 ranks = 101 + 101 + 100 -- a shorter last shard.)"""
    from test_gpu_catalogue_shard import _ns, _seen
    _spawn(_eval_worker, world, kw, str(tmp_path))
    z = [np.load(tmp_path / f"eval{r}.npz") for r in range(world)]
    ns = _ns(**kw)
    B = ns.batch_size
    for r in range(1, world):
        np.testing.assert_array_equal(z[0]["h_all"], z[r]["h_all"])
        np.testing.assert_array_equal(z[0]["E"], z[r]["E"])
    h = torch.from_numpy(z[0]["h_all"]).cuda()
    E = torch.from_numpy(z[0]["E"]).cuda()
    assert tuple(E.shape) == (ns.item_size, ns.hidden_size) and tuple(h.shape) == (world * B, ns.hidden_size)
    seen = [[int(x) for x in row] for row in _seen(ns, world * B).numpy()]      # with their -1 pads
    wi, wv = whole(h, E, seen, 20)
    ni, nv = whole(h, E, None, 20)
    for r in range(world):
        rows = slice(r * B, (r + 1) * B)
        assert_same(z[r]["fi"], z[r]["fv"], wi[rows], wv[rows], msg=f"rank {r}")                  # exact: ids and values
        assert_same(z[r]["ni"], z[r]["nv"], ni[rows], nv[rows], msg=f"rank {r}, no seen lists")
        # against the dense sharded path: bsarec_shard_logits sums in another order, near ties may swap
        np.testing.assert_allclose(z[r]["fv"], z[r]["dv"], rtol=1e-5, atol=1e-6)
        assert (z[r]["fi"] == z[r]["di"]).mean() > 0.99
    for r in range(1, world):
        np.testing.assert_array_equal(z[0]["vals2"], z[r]["vals2"])
    hits = np.concatenate([z[r]["fi"] == z[r]["ans_mixed"][:, None] for r in range(world)])
    want_m = []
    for kk in (5, 10, 20):
        want_m += [hits[:, :kk].any(1).mean(), (hits[:, :kk] / np.log2(np.arange(kk) + 2.0)).sum(1).mean()]
    np.testing.assert_allclose(z[0]["vals2"], want_m, rtol=1e-12, atol=1e-12)


def _memory_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    from bsarec_amd.catalogue import ShardedCatalogue
    from test_gpu_catalogue_shard import _batches, _ns, _seen
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        ns = _ns(item_size=400_001, train_negatives=1024, eval_full_rank="fused")
        B = ns.batch_size
        sc = ShardedCatalogue(ns, B, dist.group.WORLD, "cuda:0")
        assert sc.logits is None and sc.h_all is None
        mine = slice(rank * B, (rank + 1) * B)
        ids, ans = _batches(ns, 1, world * B)[0]
        seen = _seen(ns, world * B)
        sc.train_step(ids[mine], ans[mine])
        torch.cuda.synchronize()
        # the partial logits the dense path allocates on this rank: 200,001 rows (ld 200,004) on rank 0, 200,000 on rank 1,
        # so rank 1's quarter is the slightly tighter one
        dense_bytes = sc.Bg * sc.ld * 4
        assert dense_bytes == 64 * (200_004, 200_000)[rank] * 4
        ws_bytes = sc.lib.bsarec_topk_full_workspace_bytes(sc.Bg, sc.Vs, sc.d, 20, 0)
        before = torch.cuda.memory_allocated()
        v1, i1 = sc.topk(ids[mine], 20, seen[mine])
        torch.cuda.synchronize()
        grown = torch.cuda.memory_allocated() - before                 # what the first evaluation keeps: workspace, h_all, v1, i1
        assert sc.logits is None
        # the second evaluation: its peak above what is held when it starts (the shard's gradient and moments, torch tensors of
        # 51 MB each, are held throughout and are not the evaluation's)
        torch.cuda.reset_peak_memory_stats()
        held = torch.cuda.memory_allocated()
        v2, i2 = sc.topk(ids[mine], 20, seen[mine])
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - held
        print(f"rank {rank}: dense logits {dense_bytes} B, workspace {ws_bytes} B, first topk grew {grown} B, second topk peak {peak} B")
        assert sc.logits is None
        assert 0 < ws_bytes <= grown < dense_bytes // 4, (ws_bytes, grown, dense_bytes)
        assert peak < dense_bytes // 4, (peak, dense_bytes)
        assert torch.equal(i1, i2) and torch.equal(v1, v2)
        sc.train_step(ids[mine], ans[mine])
        sc.topk(ids[mine], 100, seen[mine])
        assert sc.logits is None
        np.savez(os.path.join(out_dir, f"mem{rank}.npz"), grown=grown, peak=peak, dense=dense_bytes, ws=ws_bytes)
        sc.close()
    finally:
        dist.destroy_process_group()


def test_fused_evaluation_under_the_sampled_head_never_holds_the_logits(tmp_path):
    """W = 2, 400,001 items, d = 64, B = 32, train_negatives = 1,024: the dense path's partial logits are 64 x 200,004 x 4 =
    51 MB per rank, the fused workspace about 3 MB.  After a training step, the first fused topk leaves memory_allocated
    less than a quarter of those 51 MB higher, a second one peaks less than a quarter of them above its start, and
    ``logits`` stays None.  (The quarter is a condition, not a measurement: the workspace alone is about 6 % of the matrix.)"""
    _spawn(_memory_worker, 2, str(tmp_path))
    for r in range(2):
        m = np.load(tmp_path / f"mem{r}.npz")
        assert 0 < int(m["ws"]) <= int(m["grown"]) < int(m["dense"]) // 4 and int(m["peak"]) < int(m["dense"]) // 4
