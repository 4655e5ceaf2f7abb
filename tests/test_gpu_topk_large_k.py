"""Exact top-k up to k = BSAREC_TOPK_MAX (1024) and evaluation at cutoffs beyond 20.

* ``bsarec_topk_seen`` against a numpy reference that builds the defined order explicitly: score descending with every NaN
  equal and above +inf, -0 == +0, equal scores by ascending column (``np.lexsort`` on column and the canonicalised key) --
  indices and values (bit patterns) exactly, plus the masked score rows;
* ``Trainer`` evaluation with ``extra_ks = (50, 100)``: the reference's six values unchanged, HR / NDCG@50 / 100 equal to
  src/metrics.py's formulas over top-100 lists from ``model.full_logits`` + masking + a stable sort;
* ``ShardedCatalogue.topk`` / ``full_sort_scores`` on two and three ranks of one GPU against the full score table.
"""
import argparse
import os
import socket

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


# ---- the reference order ---------------------------------------------------------------------------------------------------
def canon_key(x):
    """float32 -> uint32 key whose unsigned order is the defined score order (one NaN above +inf, -0 == +0)."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).copy()
    u[np.isnan(x)] = 0x7FC00000
    u[u == 0x80000000] = 0
    return np.where(u & 0x80000000, ~u, u | 0x80000000).astype(np.uint32)


def ref_topk(rows, V, k):
    """rows [B, >= V] float32 -> (idx [B, k], val [B, k]): stable descending order of rows[:, :V]."""
    idx = np.empty((rows.shape[0], k), dtype=np.int64)
    for b in range(rows.shape[0]):
        key = canon_key(rows[b, :V]).astype(np.int64)
        idx[b] = np.lexsort((np.arange(V), -key))[:k]          # last key primary: key descending, then column ascending
    return idx, np.take_along_axis(rows[:, :V], idx, axis=1)


def run_topk(rows, V, k, seen=None):
    """bsarec_topk_seen on a copy of rows [B, ld] (ld = rows.shape[1]); seen: list of item-id arrays per row, or None.
    Returns (idx, val, masked rows) as numpy."""
    from bsarec_amd import _lib as Lb
    lib = Lb.load()
    B, ld = rows.shape
    work = torch.from_numpy(np.ascontiguousarray(rows, dtype=np.float32)).cuda()
    idx = torch.full((B, k), -1, dtype=torch.int64, device="cuda")
    val = torch.empty(B, k, dtype=torch.float32, device="cuda")
    users = indptr = indices = None
    if seen is not None:
        perm = np.random.default_rng(B).permutation(B)                    # user b's CSR row is perm[b]
        csr = [None] * B
        for b in range(B):
            csr[perm[b]] = np.asarray(seen[b], dtype=np.int64)
        indptr = torch.as_tensor(np.concatenate([[0], np.cumsum([len(r) for r in csr])]).astype(np.int64), device="cuda")
        indices = torch.as_tensor(np.concatenate(csr + [np.zeros(0, np.int64)]).astype(np.int64), device="cuda")
        users = torch.as_tensor(perm.astype(np.int64), device="cuda")
    ptr = lambda t: None if t is None else t.data_ptr()
    Lb.check(lib.bsarec_topk_seen(work.data_ptr(), ld, B, V, ptr(users), ptr(indptr), ptr(indices), k, idx.data_ptr(),
                                  val.data_ptr(), torch.cuda.current_stream().cuda_stream), "bsarec_topk_seen")
    torch.cuda.synchronize()
    return idx.cpu().numpy(), val.cpu().numpy(), work.cpu().numpy()


def check(rows, V, k, seen=None):
    want_rows = np.array(rows, dtype=np.float32, copy=True)
    if seen is not None:
        for b, s in enumerate(seen):
            want_rows[b, np.asarray(s, dtype=np.int64)] = 0.0
    got_i, got_v, got_rows = run_topk(rows, V, k, seen)
    want_i, want_v = ref_topk(want_rows, V, k)
    assert np.array_equal(got_rows.view(np.uint32), want_rows.view(np.uint32))       # masking, pad columns untouched
    assert got_i.min() >= 0 and got_i.max() < V
    for b in range(len(rows)):
        assert np.array_equal(got_i[b], want_i[b]), (b, np.nonzero(got_i[b] != want_i[b])[0][:5], got_i[b][:8], want_i[b][:8])
    assert np.array_equal(got_v.view(np.uint32), want_v.view(np.uint32))               # exactly as stored (NaN payloads too)
    np.testing.assert_array_equal(got_v, want_v)                                       # (equal_nan)
    return got_i


# ---- random rows -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("V,B,k", [(3417, 256, 100), (1000, 7, 25), (40, 5, 40), (20034, 33, 1024), (100003, 3, 500),
                                   (2 ** 20 + 3, 4, 1024)])
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "seen"])
@pytest.mark.parametrize("pad", [0, 7], ids=["ld=V", "ld>V"])
def test_topk_large_k_equals_the_defined_order(V, B, k, masked, pad):
    rng = np.random.default_rng(V + k + pad)
    rows = rng.standard_normal((B, V + pad)).astype(np.float32)
    rows[::2] = np.round(rows[::2] * 16) / 16                     # every other row: many exact ties
    if pad:
        rows[:, V:] = np.where(np.arange(pad) % 2 == 0, np.inf, np.nan)   # never read
    seen = None
    if masked:
        seen = [np.unique(rng.integers(0, V, size=int(rng.integers(0, min(V, 2 * k + 50))))) for _ in range(B)]
    check(rows, V, k, seen)


# ---- adversarial rows ------------------------------------------------------------------------------------------------------
KS = (1, 20, 24, 25, 100, 1024)


def _each_k(rows, V, seen=None):
    for k in KS:
        if k <= V:
            check(rows, V, k, seen)


def test_all_scores_equal():
    rows = np.full((3, 5000), 1.5, dtype=np.float32)
    rows[1] = 0.0
    rows[2] = -np.inf
    _each_k(rows, 5000)


def test_more_seen_zeros_than_k():
    rng = np.random.default_rng(1)
    V = 4000
    rows = -np.abs(rng.standard_normal((4, V))).astype(np.float32) - 0.5             # all negative: the zeros rank first
    rows[:, :30] = 1.0                                                                # ... after 30 positives
    seen = [np.unique(rng.integers(0, V, size=1500)) for _ in range(4)]
    _each_k(rows, V, seen)


def test_tie_group_straddles_the_kth_place():
    rng = np.random.default_rng(2)
    V = 6000
    rows = rng.uniform(-1, 0.5, size=(4, V)).astype(np.float32)
    for b in range(4):
        pos = rng.permutation(V)
        rows[b, pos[:60]] = 3.0                                                       # 60 above ...
        rows[b, pos[60:60 + 2000]] = 2.0                                              # ... then 2000 equal ones
    _each_k(rows, V)


def test_values_one_ulp_apart_across_every_radix_digit():
    """Keys that differ by 1 in each byte position (and across byte carries), both signs, shuffled."""
    rng = np.random.default_rng(3)
    offs = np.unique(np.concatenate([np.arange(-300, 300)] + [d + np.arange(-3, 4) for d in (1 << 8, 1 << 16, 1 << 24, -(1 << 8), -(1 << 16), -(1 << 24))]))
    rows = []
    for base in (np.float32(1.0), np.float32(-1.0), np.float32(1e-38), np.float32(3e38)):
        b = np.array([base], dtype=np.float32).view(np.int32)[0]
        bits = (np.int64(b) + offs).astype(np.int64)
        bits = bits[(bits >= np.iinfo(np.int32).min) & (bits <= np.iinfo(np.int32).max)].astype(np.int32)
        vals = bits.view(np.float32)
        vals = vals[np.isfinite(vals)]
        rows.append(rng.permutation(np.resize(vals, 2000)))                          # (resize repeats: exact duplicates too)
    _each_k(np.stack(rows).astype(np.float32), 2000)


def test_mixed_signed_zeros_and_infinities():
    rng = np.random.default_rng(4)
    V = 3000
    choice = np.array([0.0, -0.0, np.inf, -np.inf, 1e-45, -1e-45, 1.0, -1.0], dtype=np.float32)
    rows = choice[rng.integers(0, len(choice), size=(5, V))]
    rows[4] = np.where(np.arange(V) % 2 == 0, np.float32(-0.0), np.float32(0.0))     # only zeros of both signs
    _each_k(rows, V)
    seen = [np.arange(b, V, 7) for b in range(5)]                                     # -0 / +0 mixed with the masked +0
    _each_k(rows, V, seen)


def test_nan_rows():
    """A row of NaNs (several payloads), a row with fewer than k non-NaN scores, NaN beside +inf."""
    rng = np.random.default_rng(5)
    V = 2100
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FFFFFFF], dtype=np.uint32).view(np.float32)
    rows = rng.standard_normal((3, V)).astype(np.float32)
    rows[0] = nans[rng.integers(0, len(nans), size=V)]
    rows[1] = np.nan
    rows[1, rng.permutation(V)[:15]] = rng.standard_normal(15).astype(np.float32)     # 15 comparable scores
    rows[2, rng.permutation(V)[:40]] = nans[rng.integers(0, len(nans), size=40)]
    rows[2, :10] = np.inf
    _each_k(rows, V)


def test_k20_row_with_nan_gives_valid_indices():
    """k = 20 (the per-thread list kernel): NaN ranks first, and a row with fewer than 20 comparable scores still yields
    20 in-range indices (it used to emit 0x7fffffff)."""
    rng = np.random.default_rng(6)
    V = 500
    rows = rng.standard_normal((2, V)).astype(np.float32)
    rows[0, 123] = np.nan
    rows[1, 5:] = np.nan
    idx = check(rows, V, 20)
    assert idx[0, 0] == 123 and list(idx[1]) == list(range(5, 25))


def test_rejects_k_above_the_limit_and_above_V():
    from bsarec_amd import _lib as Lb
    lib = Lb.load()
    rows = torch.zeros(2, 2000, device="cuda")
    idx = torch.empty(2, 1025, dtype=torch.int64, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    assert lib.bsarec_topk_seen(rows.data_ptr(), 2000, 2, 2000, None, None, None, 1025, idx.data_ptr(), None, st) == -10
    assert lib.bsarec_topk_seen(rows.data_ptr(), 2000, 2, 30, None, None, None, 31, idx.data_ptr(), None, st) == -10
    assert Lb.TOPK_MAX == 1024


# ---- Trainer evaluation at extra cutoffs ----------------------------------------------------------------------------------
def _ns(**kw):
    a = argparse.Namespace(item_size=301, hidden_size=64, max_seq_length=50, batch_size=128, hidden_dropout_prob=0.0,
                           attention_probs_dropout_prob=0.0, num_hidden_layers=2, num_attention_heads=2,
                           hidden_act="gelu", initializer_range=0.02, c=3, alpha=0.9, seed=42, lr=1e-3,
                           adam_beta1=0.9, adam_beta2=0.999, weight_decay=0.0, no_cuda=False, log_freq=1)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _metrics(lists, answers, ks):
    """src/metrics.py:3-31 (recall_at_k / ndcg_k) for one relevant item per user."""
    out = []
    for k in ks:
        hit = lists[:, :k] == answers[:, None]
        out += [hit.any(1).mean(), (hit / np.log2(np.arange(k) + 2.0)).sum(1).mean()]
    return out


def test_trainer_eval_with_extra_cutoffs():
    import scipy.sparse as sp
    from bsarec_amd import BSARecModel, data as D
    from bsarec_amd.trainer import Trainer
    rng = np.random.default_rng(7)
    V, L = 301, 50
    seqs = [rng.integers(1, V, size=int(rng.integers(4, 60))).tolist() for _ in range(300)]
    a = _ns(item_size=V)
    indptr, cols = D.seen_csr(seqs, "valid")
    a.valid_rating_matrix = sp.csr_matrix((np.ones(len(cols)), cols, indptr), shape=(len(seqs), V))
    users, ins, ans = D.eval_table(seqs, L, "valid")
    eval_dl = D.DeviceBatches(users, ins, ans, a.batch_size, torch.device("cuda", 0), shuffle=False)
    torch.manual_seed(11)
    model = BSARecModel(a).cuda()
    tr = Trainer(model, None, eval_dl, None, a, None)
    base, base_txt = tr.valid(0)
    a.extra_ks = (50, 100)
    got, txt = tr.valid(0)
    assert len(base) == 6 and len(got) == 10
    assert got[:6] == base                                                   # the reference's six values, exactly
    assert txt.startswith(base_txt[:-1] + ", 'HR@50': ")
    # top-100 lists from the model's own logits + masking + a stable sort
    lists = []
    with torch.no_grad():
        for s in range(0, len(seqs), a.batch_size):
            sc = model.full_logits(torch.from_numpy(ins[s:s + a.batch_size]).cuda()).cpu().numpy().copy()
            for r in range(sc.shape[0]):
                u = users[s + r]
                sc[r, cols[indptr[u]:indptr[u + 1]]] = 0.0
            lists.append(np.argsort(-sc, axis=1, kind="stable")[:, :100])
    lists = np.concatenate(lists)
    want = _metrics(lists, ans, (5, 10, 20, 50, 100))
    np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-12)


# ---- sharded catalogue, ranks on one GPU -----------------------------------------------------------------------------------
def _sharded_inputs(ns, Bg):
    g = torch.Generator(device="cpu").manual_seed(5)
    V, Lq = ns.item_size, ns.max_seq_length
    ids = torch.randint(1, V, (Bg, Lq), generator=g)
    pad = torch.randint(0, Lq - 2, (Bg,), generator=g)
    ids[torch.arange(Lq)[None, :] < pad[:, None]] = 0
    seen = torch.randint(1, V, (Bg, 40), generator=g)
    seen[:, 30:] = -1
    return ids, seen


def _shard_worker(rank, world, port, kw, ks, out_dir):
    import torch.distributed as dist
    from bsarec_amd import BSARecModel
    from bsarec_amd.catalogue import ShardedCatalogue
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        ns = _ns(**kw)
        B = ns.batch_size
        sc = ShardedCatalogue(ns, B, dist.group.WORLD, "cuda:0")
        torch.manual_seed(3)
        sc.load_full_state_dict(BSARecModel(ns).cuda().state_dict())
        ids, seen = _sharded_inputs(ns, world * B)
        mine = slice(rank * B, (rank + 1) * B)
        res = {}
        for k in ks:
            tv, ti = sc.topk(ids[mine], k, seen[mine])
            res[f"v{k}"], res[f"i{k}"] = tv.cpu().numpy(), ti.cpu().numpy()
        res["scores"] = sc.logits[:, :sc.Vs].cpu().numpy()                 # this rank's masked scores of ALL Bg sequences
        ans = torch.from_numpy(res[f"i{ks[0]}"][np.arange(B), (np.arange(B) * 7 + rank * 3) % ks[0]]).cuda()
        res["ans"] = ans.cpu().numpy()
        res["six"], _ = sc.full_sort_scores([(ids[mine], ans, seen[mine])], epoch=1)
        res["ext"], res["txt"] = sc.full_sort_scores([(ids[mine], ans, seen[mine])], epoch=1, extra_ks=(50, 100))
        np.savez(os.path.join(out_dir, f"r{rank}.npz"), **{k: np.asarray(v) for k, v in res.items()})
        sc.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,kw", [(2, dict(batch_size=32)), (3, dict(item_size=302, batch_size=16))],
                         ids=["W2", "W3_uneven_shards"])
def test_sharded_topk_large_k_equals_the_full_table(world, kw, tmp_path):
    """(W3: 302 items over 3 ranks = 101 + 101 + 100; k = V takes more candidates than any shard holds.)"""
    import torch.multiprocessing as mp
    ns = _ns(**kw)
    V, B = ns.item_size, ns.batch_size
    ks = (100, 200, V)                                       # 200 and V reach into the tie group of the seen zeros
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    mp.spawn(_shard_worker, args=(world, port, kw, ks, str(tmp_path)), nprocs=world, join=True)
    res = [dict(np.load(tmp_path / f"r{r}.npz")) for r in range(world)]
    full = np.concatenate([r["scores"] for r in res], axis=1)               # [Bg, V]: the sharded path's own scores
    assert full.shape == (world * B, V)
    # the shards' scores are the full table's (another kernel: a tolerance), with the seen items at exactly 0
    from bsarec_amd import BSARecModel
    torch.manual_seed(3)
    model = BSARecModel(ns).cuda()
    model.eval()
    ids, seen = _sharded_inputs(ns, world * B)
    with torch.no_grad():
        want = model.full_logits(ids.cuda()).cpu().numpy().copy()
    rows = np.arange(world * B)[:, None].repeat(seen.shape[1], 1)
    ok = seen.numpy() >= 0
    want[rows[ok], seen.numpy()[ok]] = 0.0
    np.testing.assert_allclose(full, want, rtol=1e-5, atol=1e-5)
    assert np.array_equal(full[rows[ok], seen.numpy()[ok]], np.zeros(ok.sum(), np.float32))
    for k in ks:
        wi, wv = ref_topk(full, V, k)
        for r in range(world):
            assert np.array_equal(res[r][f"i{k}"], wi[r * B:(r + 1) * B]), (k, r)
            assert np.array_equal(res[r][f"v{k}"], wv[r * B:(r + 1) * B]), (k, r)
    lists = np.concatenate([res[r][f"i{ks[-1]}"] for r in range(world)])
    answers = np.concatenate([res[r]["ans"] for r in range(world)])
    want_m = _metrics(lists, answers, (5, 10, 20, 50, 100))
    for r in range(world):
        np.testing.assert_array_equal(res[r]["ext"], res[0]["ext"])
        assert list(res[r]["ext"][:6]) == list(res[r]["six"])
        assert str(res[r]["txt"]).endswith("'HR@50': '{:.4f}', 'NDCG@50': '{:.4f}', 'HR@100': '{:.4f}', 'NDCG@100': '{:.4f}'}}".format(*want_m[6:]))
    np.testing.assert_allclose(res[0]["ext"], want_m, rtol=1e-12, atol=1e-12)
