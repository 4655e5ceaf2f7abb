"""bsarec_topk_full (the full-catalogue top-k without the B x V score matrix) against bsarec_topk_seen on the materialised
matrix and the numpy restatement: bit-exact on integer data, forced overflow, float data, position independence, special
values, graph capture, and the Trainer / CLI path on the shipped checkpoints and the sibling models."""
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


def fused(h, E, seen, k, cap=0, users=None):
    """h [B, d], E [V, d] fp32 device tensors; seen: list per user (or None)."""
    L, lib = _lib()
    B, d = h.shape
    V = E.shape[0]
    nb = lib.bsarec_topk_full_workspace_bytes(B, V, d, k, cap)
    assert nb > 0
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    idx = torch.empty(B, k, dtype=torch.int64, device="cuda")
    val = torch.empty(B, k, dtype=torch.float32, device="cuda")
    if seen is not None:
        indptr, indices = csr_of(seen)
        u = users if users is not None else torch.arange(B, device="cuda")
        ptrs = (u.data_ptr(), indptr.data_ptr(), indices.data_ptr())
    else:
        ptrs = (None, None, None)
    L.check(lib.bsarec_topk_full(h.data_ptr(), h.stride(0), E.data_ptr(), B, V, d, *ptrs, k, cap, ws.data_ptr(), nb,
                                 idx.data_ptr(), val.data_ptr(), torch.cuda.current_stream().cuda_stream), "bsarec_topk_full")
    torch.cuda.synchronize()
    return idx.cpu().numpy(), val.cpu().numpy()


def dense(S, seen, k):
    """bsarec_topk_seen on the fp32 matrix S [B, V] (device)."""
    L, lib = _lib()
    S = S.clone()
    B, V = S.shape
    idx = torch.empty(B, k, dtype=torch.int64, device="cuda")
    val = torch.empty(B, k, dtype=torch.float32, device="cuda")
    if seen is not None:
        indptr, indices = csr_of(seen)
        u = torch.arange(B, device="cuda")
        ptrs = (u.data_ptr(), indptr.data_ptr(), indices.data_ptr())
    else:
        ptrs = (None, None, None)
    L.check(lib.bsarec_topk_seen(S.data_ptr(), S.stride(0), B, V, *ptrs, k, idx.data_ptr(), val.data_ptr(),
                                 torch.cuda.current_stream().cuda_stream), "bsarec_topk_seen")
    torch.cuda.synchronize()
    return idx.cpu().numpy(), val.cpu().numpy()


def int_case(B, V, d, seed, lo=-3, hi=3, seen_kind="mixed", k=20):
    """Integer h, E (|x| <= 3) and S = h E^T, exact in fp32 (every partial sum an integer below 2^24), computed in fp64 on
    the device and kept there (S: a device tensor)."""
    rng = np.random.default_rng(seed)
    h = rng.integers(lo, hi + 1, size=(B, d)).astype(np.float32)
    E = rng.integers(-3, 4, size=(V, d)).astype(np.float32)
    S = (torch.from_numpy(h).cuda().double() @ torch.from_numpy(E).cuda().double().T).float()
    seen = None
    if seen_kind == "mixed":
        best = torch.topk(S, min(V, k + 2), dim=1).indices.cpu().numpy()
        seen = []
        for b in range(B):
            n = int(rng.integers(0, min(V, 3 * k + 5)))
            s = rng.choice(V, size=n, replace=False).tolist()
            if b % 3 == 0:                       # answers that are seen: the row's best items
                s += best[b].tolist()
            seen.append(s)
    return h, E, S, seen


def check_exact(h, E, S, seen, k, caps=(0,)):
    if not torch.is_tensor(S):
        S = torch.from_numpy(S).cuda()
    ht = h if torch.is_tensor(h) else torch.from_numpy(h).cuda()       # (a device tensor keeps its row stride)
    Et = torch.from_numpy(E).cuda()
    di, dv = dense(S, seen, k)
    if S.numel() <= 5_000_000:                   # the numpy restatement where it is quick
        ri, rv = R.topk(S.cpu().numpy(), seen if seen is not None else [[]] * S.shape[0], k)
        np.testing.assert_array_equal(di, ri)
        np.testing.assert_array_equal(dv.view(np.uint32), rv.view(np.uint32))
    for cap in caps:
        fi, fv = fused(ht, Et, seen, k, cap)
        np.testing.assert_array_equal(fi, di, err_msg=f"cap {cap}")
        np.testing.assert_array_equal(fv.view(np.uint32), dv.view(np.uint32), err_msg=f"cap {cap}")


CASES = [  # (B, V, d, k)
    (1, 20, 16, 20), (3, 1000, 64, 1), (3, 1000, 16, 100), (257, 4097, 64, 20), (256, 4097, 256, 1024), (3, 1024, 64, 1024),
    (256, 100_003, 64, 20), (3, 100_003, 256, 100), (256, 1_000_003, 64, 20), (3, 1_000_003, 16, 1024), (2, 1_000_003, 64, 100),
]


@pytest.mark.parametrize("B,V,d,k", CASES)
def test_bit_exact_against_dense_on_integer_data(B, V, d, k):
    h, E, S, seen = int_case(B, V, d, seed=B * 7 + V + k, k=k)
    check_exact(h, E, S, seen, k)
    check_exact(h, E, S, None, k)


@pytest.mark.parametrize("B,V,d,k", [(3, 1000, 64, 20), (257, 4097, 16, 100), (3, 100_003, 64, 20), (4, 4097, 64, 1024)])
def test_forced_overflow_gives_identical_lists(B, V, d, k):
    h, E, S, seen = int_case(B, V, d, seed=11 + V, k=k)
    check_exact(h, E, S, seen, k, caps=(0, k, k + 37 if (k + 37) % 2 else k + 38, 4 * k + 1))


def test_row_stride_not_a_multiple_of_four():
    """h = wide[:, :d] of a (B, d + 1) buffer whose pad column holds 99: the tile is staged float by float.  130 rows: a full
    row tile and one of two rows; 300 items: two full item blocks and a tail whose second wave is part-filled and whose third
    and fourth are empty; d = 68: a k count that is no multiple of 32."""
    B, V, d, k = 130, 300, 68, 20
    h, E, S, seen = int_case(B, V, d, seed=23, k=k)
    wide = torch.full((B, d + 1), 99.0, device="cuda")
    wide[:, :d] = torch.from_numpy(h).cuda()
    hv = wide[:, :d]
    assert hv.data_ptr() % 16 == 0 and hv.stride(0) == d + 1
    check_exact(hv, E, S, seen, k)
    ci, cv = fused(torch.from_numpy(h).cuda(), torch.from_numpy(E).cuda(), seen, k)
    fi, fv = fused(hv, torch.from_numpy(E).cuda(), seen, k)
    np.testing.assert_array_equal(fi, ci)
    np.testing.assert_array_equal(fv.view(np.uint32), cv.view(np.uint32))


def test_negative_rows_seen_zeros_win_and_all_zero_table():
    h, E, S, seen = int_case(64, 5000, 64, seed=5, k=20)
    h = -np.abs(h) - 1
    E = np.abs(E) + 1                                   # every score < 0: the seen zeros come first
    S = (h.astype(np.float64) @ E.astype(np.float64).T).astype(np.float32)
    check_exact(h, E, S, seen, 20, caps=(0, 20, 41))
    check_exact(h, E, S, None, 20, caps=(0, 20))
    Z = np.zeros((5000, 64), np.float32)
    SZ = np.zeros((64, 5000), np.float32)
    check_exact(h, Z, SZ, seen, 20, caps=(0, 20))
    fi, fv = fused(torch.from_numpy(h).cuda(), torch.from_numpy(Z).cuda(), None, 100)
    assert (fi == np.arange(100)).all() and (fv == 0).all()


def test_float_data_tolerance_and_order():
    rng = np.random.default_rng(1)
    B, V, d, k = 64, 100_003, 64, 100
    h = rng.standard_normal((B, d)).astype(np.float32)
    E = (rng.standard_normal((V, d)) * 0.3).astype(np.float32)
    S64 = h.astype(np.float64) @ E.astype(np.float64).T
    seen = [rng.choice(V, size=int(rng.integers(0, 200)), replace=False).tolist() for _ in range(B)]
    fi, fv = fused(torch.from_numpy(h).cuda(), torch.from_numpy(E).cuda(), seen, k)
    for b in range(B):
        m = S64[b].copy()
        m[seen[b]] = 0
        np.testing.assert_allclose(fv[b], m[fi[b]], rtol=1e-5, atol=1e-6)
        kth = fv[b, -1]
        rest = np.ones(V, bool)
        rest[fi[b]] = False
        assert (m[rest] <= kth + 1e-5 * abs(kth) + 1e-6).all()
        assert all((fv[b, i] > fv[b, i + 1]) or (fv[b, i] == fv[b, i + 1] and fi[b, i] < fi[b, i + 1]) for i in range(k - 1))
    # forced overflow: the same list, bit for bit
    gi, gv = fused(torch.from_numpy(h).cuda(), torch.from_numpy(E).cuda(), seen, k, cap=k)
    np.testing.assert_array_equal(gi, fi)
    np.testing.assert_array_equal(gv.view(np.uint32), fv.view(np.uint32))


def test_position_independence_prefix_and_determinism():
    rng = np.random.default_rng(2)
    B, V, d = 40, 20_011, 64
    h = rng.standard_normal((B, d)).astype(np.float32)
    E = rng.standard_normal((V, d)).astype(np.float32)
    seen = [rng.choice(V, size=int(rng.integers(0, 50)), replace=False).tolist() for _ in range(B)]
    ht, Et = torch.from_numpy(h).cuda(), torch.from_numpy(E).cuda()
    i1, v1 = fused(ht, Et, seen, 50)
    i2, v2 = fused(ht, Et, seen, 50)
    np.testing.assert_array_equal(i1, i2)
    np.testing.assert_array_equal(v1.view(np.uint32), v2.view(np.uint32))
    i3, v3 = fused(ht, Et, seen, 20)
    np.testing.assert_array_equal(i3, i1[:, :20])
    np.testing.assert_array_equal(v3.view(np.uint32), v1[:, :20].view(np.uint32))
    pb, pv = rng.permutation(B), rng.permutation(V)     # row and item permutations (item j moves to inv[j])
    inv = np.empty(V, np.int64)
    inv[pv] = np.arange(V)
    seen_p = [[int(inv[j]) for j in seen[b]] for b in pb]
    i4, v4 = fused(torch.from_numpy(h[pb]).cuda(), torch.from_numpy(np.ascontiguousarray(E[pv])).cuda(), seen_p, 50)
    np.testing.assert_array_equal(pv[i4], i1[pb])
    np.testing.assert_array_equal(v4.view(np.uint32), v1[pb].view(np.uint32))


def test_special_values():
    rng = np.random.default_rng(4)
    B, V, d, k = 8, 3000, 64, 20
    h = rng.integers(-3, 4, size=(B, d)).astype(np.float32)
    E = rng.integers(-3, 4, size=(V, d)).astype(np.float32)
    E[1234, 5] = np.nan                                  # a NaN item ranks first in every row
    h[3, :] = np.nan                                     # a NaN row: every score NaN -> columns 0..k-1
    S = np.full((B, V), np.nan, np.float32)
    with np.errstate(invalid="ignore"):
        S[:] = (h.astype(np.float64) @ E.astype(np.float64).T).astype(np.float32)
    fi, fv = fused(torch.from_numpy(h).cuda(), torch.from_numpy(E).cuda(), None, k)
    di, dv = dense(torch.from_numpy(S).cuda(), None, k)
    np.testing.assert_array_equal(fi, di)
    assert (fi[[0, 1, 2, 4, 5, 6, 7], 0] == 1234).all()
    assert (fi[3] == np.arange(k)).all() and np.isnan(fv[3]).all()
    # -0 ties with a seen +0: column order decides
    h2 = np.zeros((1, 4), np.float32)
    h2[0, 0] = -1.0
    E2 = np.zeros((40, 4), np.float32)
    E2[:, 0] = -1.0                                      # all scores +1 ...
    E2[5:30, 0] = 0.0                                    # ... except -0 * ... = -0 / +0 for columns 5..29
    E2[7, 0] = 2.0                                       # column 7: -2, but seen -> +0
    fi, fv = fused(torch.from_numpy(h2).cuda(), torch.from_numpy(E2).cuda(), [[7]], 20)
    S2 = (h2 @ E2.T).astype(np.float32)
    ri, rv = R.topk(S2, [[7]], 20)
    np.testing.assert_array_equal(fi, ri)
    di, dv = dense(torch.from_numpy(S2).cuda(), [[7]], 20)
    np.testing.assert_array_equal(fi, di)
    np.testing.assert_array_equal(fv.view(np.uint32), dv.view(np.uint32))


def test_graph_capture_replays_and_allocates_nothing():
    L, lib = _lib()
    rng = np.random.default_rng(6)
    B, V, d, k = 64, 50_000, 64, 20
    h = torch.from_numpy(rng.standard_normal((B, d)).astype(np.float32)).cuda()
    E = torch.from_numpy(rng.standard_normal((V, d)).astype(np.float32)).cuda()
    seen = [rng.choice(V, size=30, replace=False).tolist() for _ in range(B)]
    indptr, indices = csr_of(seen)
    users = torch.arange(B, device="cuda")
    nb = lib.bsarec_topk_full_workspace_bytes(B, V, d, k, 0)
    ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
    idx = torch.empty(B, k, dtype=torch.int64, device="cuda")
    val = torch.empty(B, k, dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()

    def call(stream):
        L.check(lib.bsarec_topk_full(h.data_ptr(), d, E.data_ptr(), B, V, d, users.data_ptr(), indptr.data_ptr(),
                                     indices.data_ptr(), k, 0, ws.data_ptr(), nb, idx.data_ptr(), val.data_ptr(),
                                     stream.cuda_stream), "bsarec_topk_full")
    with torch.cuda.stream(s):
        call(s)                                          # eager warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    with torch.cuda.stream(s):
        call(s)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() == base
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(s)
    torch.cuda.synchronize()
    h.copy_(torch.from_numpy(rng.standard_normal((B, d)).astype(np.float32)))
    E.copy_(torch.from_numpy(rng.standard_normal((V, d)).astype(np.float32)))
    g.replay()
    torch.cuda.synchronize()
    gi, gv = idx.cpu().numpy(), val.cpu().numpy()
    ei, ev = fused(h, E, seen, k)
    np.testing.assert_array_equal(gi, ei)
    np.testing.assert_array_equal(gv.view(np.uint32), ev.view(np.uint32))


def _kat_trainer(name, **extra):
    import scipy.sparse as sp
    from bsarec_amd import BSARecModel, data as D
    from bsarec_amd.trainer import Trainer
    from test_gpu_boundary import load_kat, ns
    z, cfg, seqs = load_kat(name)
    a = ns(item_size=cfg["item_size"], num_attention_heads=cfg["num_attention_heads"], c=cfg["c"], alpha=cfg["alpha"], **extra)
    model = BSARecModel(a)
    model.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p/")})
    model = model.cuda()
    model.eval()
    users, ins, ans = D.eval_table(seqs, 50, "test")
    indptr, cols = D.seen_csr(seqs, "test")
    a.train_matrix = sp.csr_matrix((np.ones(len(cols)), cols, indptr), shape=(len(seqs), cfg["item_size"]))
    return z, Trainer(model, None, None, None, a, None), ins


@pytest.mark.parametrize("name", ["LastFM", "Beauty"])
def test_shipped_checkpoint_top20_lists(name):
    """As test_gpu_boundary.test_shipped_checkpoint_top20_lists, through Trainer.topk_full; and equal to the dense path's
    lists under the same near-tie rule."""
    z, tr, ins = _kat_trainer(name)
    u, x = torch.arange(64, device="cuda"), torch.from_numpy(ins[:64]).cuda()
    pred, scores = tr.topk_full(u, x, return_scores=True)
    pred, sc = pred.cpu().numpy(), scores.cpu().numpy()
    want = z["top20_64"].astype(np.int64)
    dpred, dense_scores = tr.topk_after_seen(u, x, return_scores=True)
    ds = dense_scores.cpu().numpy()
    for ref in (want, dpred.cpu().numpy()):
        for b, r in zip(*np.nonzero(pred != ref)):
            assert abs(ds[b, pred[b, r]] - ds[b, ref[b, r]]) < 2e-5, (b, r, pred[b], ref[b])
        assert (pred != ref).mean() < 0.01
    np.testing.assert_array_equal(pred[:, :10], want[:, :10])
    np.testing.assert_allclose(sc, np.take_along_axis(ds, pred, axis=1), rtol=1e-5, atol=1e-6)


def test_do_eval_cli_with_fused_full_rank(tmp_path):
    """`main --do_eval --eval_full_rank fused` reproduces the shipped checkpoint's logged LastFM test metrics."""
    from bsarec_amd import data as D, main as M
    from test_gpu_boundary import load_kat
    z, _tr, _ = _kat_trainer("LastFM")
    _tr.save(str(tmp_path / "BSARec_LastFM_fr.pt"))
    _, cfg, seqs = load_kat("LastFM")
    D.write_user_seqs(str(tmp_path / "LastFM.txt"), seqs)
    res = M.main(["--data_dir", str(tmp_path) + "/", "--data_name", "LastFM", "--output_dir", str(tmp_path) + "/",
                  "--do_eval", "--load_model", "BSARec_LastFM_fr", "--train_name", "fr_eval", "--eval_full_rank", "fused",
                  "--num_attention_heads", str(cfg["num_attention_heads"]), "--c", str(cfg["c"]), "--alpha", str(cfg["alpha"])])
    np.testing.assert_allclose(res[0], z["metrics"], rtol=0, atol=1e-12)


@pytest.mark.parametrize("model_type", ["SASRec", "FMLPRec"])
def test_siblings_through_trainer_iteration(model_type):
    """Trainer.iteration's full-sort branch with --eval_full_rank fused gives the dense path's lists (near-tie rule)."""
    import scipy.sparse as sp
    from bsarec_amd import MODEL_DICT, data as D, main as M
    from bsarec_amd.trainer import Trainer
    from test_gpu_boundary import load_kat
    _, cfg, seqs = load_kat("LastFM")
    args = M.parse_args(["--model_type", model_type, "--num_attention_heads", "1"])
    args.item_size = cfg["item_size"]
    torch.manual_seed(0)
    model = MODEL_DICT[model_type.lower()](args=args).cuda()
    users, ins, ans = D.eval_table(seqs, args.max_seq_length, "test")
    indptr, cols = D.seen_csr(seqs, "test")
    args.train_matrix = sp.csr_matrix((np.ones(len(cols)), cols, indptr), shape=(len(seqs), cfg["item_size"]))
    n = 300
    batches = [(torch.from_numpy(users[i:i + 128]), torch.from_numpy(ins[i:i + 128]), torch.from_numpy(ans[i:i + 128]),
                torch.zeros(1), torch.zeros(1)) for i in range(0, n, 128)]
    tr = Trainer(model, None, None, None, args, None)
    got = {}

    def grab(epoch, answers, pred_list, extra_ks=None):
        got["pred"] = pred_list.cpu().numpy() if hasattr(pred_list, "cpu") else np.asarray(pred_list)
        return [0.0] * 6, ""
    tr.get_full_sort_score = grab
    tr.iteration(0, batches, train=False)
    want = got["pred"]
    args.eval_full_rank = "fused"
    tr.iteration(0, batches, train=False)
    pred = got["pred"]
    x = torch.from_numpy(ins[:n]).cuda()
    _, ds = tr.topk_after_seen(torch.from_numpy(users[:n]).cuda(), x, return_scores=True)
    ds = ds.cpu().numpy()
    for b, r in zip(*np.nonzero(pred != want)):
        assert abs(ds[b, pred[b, r]] - ds[b, want[b, r]]) < 2e-5, (b, r)
    assert (pred != want).mean() < 0.01
