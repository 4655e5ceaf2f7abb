"""bsarec_answer_rank / bsarec_answer_rank_range / bsarec_answer_score_range (the answer's exact full-catalogue rank without a
score matrix or a list) against the numpy restatement (bit for bit on integer data), against the list kernels on float data
(FullRank with k = V; bsarec_topk_seen's 1024-list), the corners of the contract, the additivity over ranges, graph capture,
and Trainer's eval_full_rank = "rank"."""
import numpy as np
import pytest

import answer_rank_ref as A

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


def _seen_ptrs(seen, B):
    if seen is None:
        return (None, None, None), None
    indptr, indices = csr_of(seen)
    users = torch.arange(B, device="cuda")
    return (users.data_ptr(), indptr.data_ptr(), indices.data_ptr()), (users, indptr, indices)


def rank_range(h, E, seen, answers, base=0, answer_score=None, scores=True, entry="range"):
    """(ranks int32 [B], scores fp32 [B] or None) of the rows E = rows [base, base + len(E)) of a catalogue; seen: GLOBAL ids."""
    L, lib = _lib()
    B, d = h.shape
    ptrs, keep = _seen_ptrs(seen, B)
    ans = torch.as_tensor(np.asarray(answers, np.int64)).cuda()
    given = None if answer_score is None else torch.as_tensor(np.asarray(answer_score, np.float32)).cuda()
    rank = torch.full((B,), -7, dtype=torch.int32, device="cuda")
    val = torch.full((B,), -7.0, dtype=torch.float32, device="cuda") if scores else None
    st = torch.cuda.current_stream().cuda_stream
    vp = None if val is None else val.data_ptr()
    if entry == "whole":
        assert base == 0 and given is None
        L.check(lib.bsarec_answer_rank(h.data_ptr(), h.stride(0), E.data_ptr(), B, E.shape[0], d, *ptrs, ans.data_ptr(),
                                       rank.data_ptr(), vp, st), "bsarec_answer_rank")
    else:
        L.check(lib.bsarec_answer_rank_range(h.data_ptr(), h.stride(0), E.data_ptr(), B, E.shape[0], base, d, *ptrs, ans.data_ptr(),
                                             None if given is None else given.data_ptr(), rank.data_ptr(), vp, st),
                "bsarec_answer_rank_range")
    torch.cuda.synchronize()
    return rank.cpu().numpy(), None if val is None else val.cpu().numpy()


def score_range(h, E, seen, answers, base, out):
    L, lib = _lib()
    B, d = h.shape
    ptrs, keep = _seen_ptrs(seen, B)
    ans = torch.as_tensor(np.asarray(answers, np.int64)).cuda()
    L.check(lib.bsarec_answer_score_range(h.data_ptr(), h.stride(0), E.data_ptr(), B, E.shape[0], base, d, *ptrs, ans.data_ptr(),
                                          out.data_ptr(), torch.cuda.current_stream().cuda_stream), "bsarec_answer_score_range")
    torch.cuda.synchronize()
    return out


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def assert_same(got, want, msg=""):
    np.testing.assert_array_equal(got[0], want[0], err_msg=msg)
    if got[1] is not None:
        np.testing.assert_array_equal(bits(got[1]), bits(want[1]), err_msg=msg)


def int_case(B, V, d, seed):
    """Integer h, E (|x| <= 3): S = h E^T is exact in fp32 in every summation order.  Seen rows: unsorted, with repeats, pads and
    ids outside the catalogue; rows b % 3 == 0 have seen their answer, rows b % 3 == 1 answer one of their row's best items."""
    rng = np.random.default_rng(seed)
    h = rng.integers(-3, 4, size=(B, d)).astype(np.float32)
    E = rng.integers(-3, 4, size=(V, d)).astype(np.float32)
    S = (h.astype(np.float64) @ E.astype(np.float64).T).astype(np.float32) + np.float32(0.0)      # (no -0: the chain starts at +0)
    answers = rng.integers(0, V, size=B)
    best = np.argsort(-S, axis=1, kind="stable")
    seen = []
    for b in range(B):
        if b % 3 == 1:
            answers[b] = best[b, int(rng.integers(0, min(V, 5)))]
        s = rng.integers(0, V, size=int(rng.integers(0, min(V, 65)))).tolist()
        s += s[: len(s) // 3] + best[b, :3].tolist() + [-1, V, V + 11, -5]
        if b % 3 == 0:
            s += [int(answers[b])] * 2
        rng.shuffle(s)
        seen.append([int(x) for x in s])
    return h, E, S, seen, answers


@pytest.mark.parametrize("d", [4, 64, 68, 256])
@pytest.mark.parametrize("V", [40, 127, 129, 4099])
@pytest.mark.parametrize("B", [1, 5, 130])
def test_bit_exact_against_the_reference_on_integer_data(B, V, d):
    h, E, S, seen, answers = int_case(B, V, d, seed=B * 7 + V + d)
    ht, Et = torch.from_numpy(h).cuda(), torch.from_numpy(E).cuda()
    for sn in (seen, None):
        want = A.ranks(S, sn if sn is not None else [[]] * B, answers)
        assert_same(rank_range(ht, Et, sn, answers, entry="whole"), want, "bsarec_answer_rank")
        assert_same(rank_range(ht, Et, sn, answers), want, "range, base 0")
        assert_same(rank_range(ht, Et, sn, answers, scores=False), want, "score_out == NULL")
    if V <= 129:
        np.testing.assert_array_equal(want[0], A.index_in_full_list(S, [[]] * B, answers))


def float_case(B, V, d, seed):
    rng = np.random.default_rng(seed)
    h = rng.standard_normal((B, d)).astype(np.float32)
    E = (rng.standard_normal((V, d)) * 0.3).astype(np.float32)
    E[rng.integers(0, V, size=max(1, V // 16))] = E[0]                # equal rows: exact ties on float data
    answers = rng.integers(0, V, size=B)
    seen = []
    for b in range(B):
        s = rng.integers(0, V, size=int(rng.integers(0, min(V, 60)))).tolist()
        if b % 4 == 0:
            s += [int(answers[b])]
        seen.append(s + s[:3])
    return torch.from_numpy(h).cuda(), torch.from_numpy(E).cuda(), seen, answers


@pytest.mark.parametrize("B,V,d", [(1, 40, 4), (5, 127, 64), (130, 129, 68), (130, 1024, 64), (5, 1000, 256)])
def test_float_data_rank_is_the_index_in_the_full_list_of_topk_full(B, V, d):
    from bsarec_amd.ranking import FullRank
    h, E, seen, answers = float_case(B, V, d, seed=V + d)
    users = torch.arange(B, device="cuda")
    for sn in (seen, None):
        idx, val = FullRank("unsupported {B} {V} {d} {k}")(h, E, V, users if sn else None, csr_of(sn) if sn else None, values=True)
        idx, val = idx.cpu().numpy(), val.cpu().numpy()
        rank, score = rank_range(h, E, sn, answers)
        for b in range(B):
            assert idx[b, rank[b]] == answers[b], (b, rank[b])
            assert bits(val[b, rank[b]]) == bits(score[b])


def _fmaf_score_matrix(h, E):
    """The raw fp32 score matrix of the kernels' fmaf chain, from FullRank over parts of at most 1024 items with k = Vs."""
    from bsarec_amd.ranking import FullRank
    B, V = h.shape[0], E.shape[0]
    S = torch.empty(B, V, dtype=torch.float32, device="cuda")
    fr = FullRank("unsupported {B} {V} {d} {k}")
    for lo in range(0, V, 1024):
        part = E[lo:lo + 1024].contiguous()
        idx, val = fr(h, part, part.shape[0], values=True)
        S[:, lo:lo + 1024].scatter_(1, idx, val)
    return S


@pytest.mark.parametrize("B,d", [(5, 64), (130, 68)])
def test_float_data_agrees_with_the_1024_list_of_topk_seen(B, d):
    from bsarec_amd.ranking import topk_seen
    V = 4099
    h, E, seen, answers = float_case(B, V, d, seed=B + d)
    for b in range(B):                                                # answers from the top and from the bottom of their rows
        sign = 1.0 if b % 2 == 0 else -1.0
        answers[b] = int(torch.topk(sign * (E @ h[b]), 900).indices[(37 * b) % 900])
    S = _fmaf_score_matrix(h, E)
    users = torch.arange(B, device="cuda")
    top = topk_seen(S.clone(), 1024, users, csr_of(seen)).cpu().numpy()
    rank, score = rank_range(h, E, seen, answers)
    inside = 0
    for b in range(B):
        where = np.nonzero(top[b] == answers[b])[0]
        assert (rank[b] < 1024) == (where.size == 1), (b, rank[b])
        if where.size:
            assert where[0] == rank[b]
            inside += 1
    assert 0 < inside < B
    np.testing.assert_array_equal(rank, A.ranks(S.cpu().numpy(), seen, answers)[0])


def test_corners():
    rng = np.random.default_rng(9)
    B, V, d = 7, 300, 64
    h = rng.integers(-3, 4, size=(B, d)).astype(np.float32)
    E = rng.integers(-3, 4, size=(V, d)).astype(np.float32)
    ht, Et = torch.from_numpy(h).cuda(), torch.from_numpy(E).cuda()
    answers = rng.integers(0, V, size=B)
    # an all-zero table: every score ties, the rank is the answer's column -- whatever is seen
    Z = torch.zeros(V, d, device="cuda")
    seen = [rng.integers(0, V, size=40).tolist() for _ in range(B)]
    for sn in (None, seen):
        rank, score = rank_range(ht, Z, sn, answers)
        np.testing.assert_array_equal(rank, answers)
        assert (bits(score) == 0).all()
    # the answer seen; a row seen almost entirely (all but three items, unsorted, every id twice); negative and out-of-range
    # entries; a row without entries
    S = (h.astype(np.float64) @ E.astype(np.float64).T).astype(np.float32)
    keep = rng.choice(V, size=3, replace=False)
    most = [int(x) for x in rng.permutation(np.setdiff1d(np.arange(V), keep))]
    seen = [[int(answers[0])], most + most[::-1], [-1, -5, V, V + 1, 2 ** 40, -2 ** 40, 2 ** 31 - 1], [],
            [int(answers[4])] * 5 + [3, 3, 1, 299, 0, 0], most + [int(keep[0])], [5, 4, 3, 3, 4, 5]]
    answers[1], answers[5] = keep[1], most[7]
    want = A.ranks(S, seen, answers)
    assert want[1][0] == 0 and want[1][4] == 0 and want[1][5] == 0
    assert_same(rank_range(ht, Et, seen, answers), want)
    assert_same(rank_range(ht, Et, seen, answers, scores=False), want)
    # ldh > d: the rows of a wider matrix
    wide = torch.zeros(B, d + 12, device="cuda")
    wide[:, :d] = ht
    wide[:, d:] = 99.0
    assert_same(rank_range(wide[:, :d], Et, seen, answers), want)
    # ldh % 4 != 0: the tile is staged float by float.  Two row tiles (128 + 2 rows), two full item blocks and a tail whose
    # second wave is part-filled, a k count (68) that is no multiple of 32
    h2, E2, S2, seen2, ans2 = int_case(130, 300, 68, seed=31)
    odd = torch.full((130, 69), 99.0, device="cuda")
    odd[:, :68] = torch.from_numpy(h2).cuda()
    assert odd.data_ptr() % 16 == 0 and odd[:, :68].stride(0) == 69
    want2 = A.ranks(S2, seen2, ans2)
    assert_same(rank_range(odd[:, :68], torch.from_numpy(E2).cuda(), seen2, ans2), want2, "ldh = d + 1")
    assert_same(rank_range(odd[:, :68], torch.from_numpy(E2).cuda(), seen2, ans2, scores=False), want2, "ldh = d + 1, no scores")
    # an answer outside [0, V): -1 and NaN, and the other rows as before
    out = answers.copy()
    out[[0, 3, 6]] = [-1, V, 2 ** 40]
    rank, score = rank_range(ht, Et, seen, out)
    assert (rank[[0, 3, 6]] == -1).all() and np.isnan(score[[0, 3, 6]]).all()
    ok = [1, 2, 4, 5]
    np.testing.assert_array_equal(rank[ok], want[0][ok])
    np.testing.assert_array_equal(bits(score[ok]), bits(want[1][ok]))
    rank, _ = rank_range(ht, Et, seen, out, scores=False)
    assert (rank[[0, 3, 6]] == -1).all() and (rank[ok] == want[0][ok]).all()


def test_nan_and_negative_zero():
    rng = np.random.default_rng(4)
    B, V, d = 8, 3000, 64
    h = rng.integers(-3, 4, size=(B, d)).astype(np.float32)
    E = rng.integers(-3, 4, size=(V, d)).astype(np.float32)
    E[1234, 5] = np.nan                                  # a NaN item stands before every other item
    h[3, :] = np.nan                                     # a NaN row: every score NaN, the column order decides
    with np.errstate(invalid="ignore"):
        S = (h.astype(np.float64) @ E.astype(np.float64).T).astype(np.float32)
    answers = np.array([1234, 7, 2999, 1500, 0, 1234, 1233, 1235])
    seen = [[], [1234], [5, 6], [], [1234, 0], [1234], [9], []]
    want = A.ranks(S, seen, answers)
    assert want[0][0] == 0 and want[0][3] == 1500 and np.isnan(want[1][0]) and want[1][5] == 0
    got = rank_range(torch.from_numpy(h).cuda(), torch.from_numpy(E).cuda(), seen, answers)
    np.testing.assert_array_equal(got[0], want[0])
    np.testing.assert_array_equal(np.isnan(got[1]), np.isnan(want[1]))
    np.testing.assert_array_equal(A.order_key(got[1]), A.order_key(want[1]))
    # -0 ties with +0 and with a seen +0: the column order decides
    h2 = np.zeros((3, 4), np.float32)
    h2[:, 0] = -1.0
    E2 = np.zeros((40, 4), np.float32)
    E2[:, 0] = -1.0                                      # all scores +1 ...
    E2[5:30, 0] = 0.0                                    # ... except -0 for columns 5 .. 29
    E2[7, 0] = 2.0                                       # column 7: -2, but seen -> +0
    S2 = (h2 @ E2.T).astype(np.float32)
    answers2, seen2 = np.array([7, 20, 2]), [[7], [7], [7]]
    want2 = A.ranks(S2, seen2, answers2)
    np.testing.assert_array_equal(want2[0], [15 + 2, 15 + 15, 2])
    got2 = rank_range(torch.from_numpy(h2).cuda(), torch.from_numpy(E2).cuda(), seen2, answers2)
    np.testing.assert_array_equal(got2[0], want2[0])
    np.testing.assert_array_equal(A.order_key(got2[1]), A.order_key(want2[1]))
    # a given score of -0.0 (the chain itself never yields one: it starts at +0) stands where +0.0 stands
    for zero in (-0.0, 0.0):
        given = np.full(3, zero, np.float32)
        want3 = A.ranks(S2, seen2, answers2, answer_score=given)
        np.testing.assert_array_equal(want3[0], [17, 30, 14])
        got3 = rank_range(torch.from_numpy(h2).cuda(), torch.from_numpy(E2).cuda(), seen2, answers2, answer_score=given)
        np.testing.assert_array_equal(got3[0], want3[0])
        np.testing.assert_array_equal(bits(got3[1]), bits(given))


def test_long_row_with_repeats_across_the_dedupe_chunks():
    """3,000 entries over V = 5,003: the kernel dedupes 2,048 entries at a time; ids repeat inside the first chunk, inside the
    second, and across the boundary -- each distinct item must count once."""
    rng = np.random.default_rng(12)
    B, V, d = 3, 5003, 64
    h = -np.abs(rng.integers(-3, 4, size=(B, d))).astype(np.float32) - 1
    E = np.abs(rng.integers(-3, 4, size=(V, d))).astype(np.float32) + 1      # every score < 0: each seen zero moves the rank
    S = (h.astype(np.float64) @ E.astype(np.float64).T).astype(np.float32)
    first = rng.choice(V, size=1500, replace=False)
    row = np.concatenate([first, first[:548], rng.choice(V, size=500, replace=False), first[600:900]])   # 2,048 | 800
    row = np.concatenate([row, row[2048:2200]])
    assert len(row) == 3000 and len(np.unique(row)) < 2000
    seen = [[int(x) for x in row], [int(x) for x in row[::-1]], [int(x) for x in rng.permutation(row)]]
    answers = np.array([int(np.setdiff1d(np.arange(V), row)[17]), int(row[2100]), int(first[3])])
    want = A.ranks(S, seen, answers)
    assert want[0][0] >= len(np.unique(row))             # an unseen answer of a negative row: behind every distinct seen item
    ht, Et = torch.from_numpy(h).cuda(), torch.from_numpy(E).cuda()
    assert_same(rank_range(ht, Et, seen, answers), want)
    assert_same(rank_range(ht, Et, seen, answers, scores=False), want)


@pytest.mark.parametrize("bounds", [[(0, 200), (200, 401)], [(0, 1), (1, 130), (130, 401)], [(0, 129), (129, 130), (130, 401)]])
@pytest.mark.parametrize("kind", ["int", "float"])
def test_ranges_sum_to_the_whole_catalogue(bounds, kind):
    B, V, d = 130, 401, 64
    if kind == "int":
        h, E, S, seen, answers = int_case(B, V, d, seed=len(bounds))
        ht, Et = torch.from_numpy(h).cuda(), torch.from_numpy(E).cuda()
    else:
        ht, Et, seen, answers = float_case(B, V, d, seed=len(bounds))
    whole = rank_range(ht, Et, seen, answers, entry="whole")
    parts = [(lo, Et[lo:hi].contiguous()) for lo, hi in bounds]
    score = torch.zeros(B, device="cuda")
    for lo, Ep in parts:
        mine = torch.zeros(B, device="cuda")
        score_range(ht, Ep, seen, answers, lo, mine)
        own = (answers >= lo) & (answers < lo + Ep.shape[0])
        assert (bits(mine.cpu().numpy())[~own] == 0).all()          # untouched
        score = score + mine
    np.testing.assert_array_equal(A.order_key(score.cpu().numpy()), A.order_key(whole[1]))
    total = np.zeros(B, np.int64)
    for lo, Ep in parts:
        r, v = rank_range(ht, Ep, seen, answers, base=lo, answer_score=score.cpu().numpy())
        assert (r >= 0).all()
        np.testing.assert_array_equal(bits(v), bits(score.cpu().numpy()))
        total += r
        # without a given score: the part ranks its own answers (the same counts) and refuses the others
        r2, v2 = rank_range(ht, Ep, seen, answers, base=lo)
        own = (answers >= lo) & (answers < lo + Ep.shape[0])
        assert (r2[~own] == -1).all() and np.isnan(v2[~own]).all()
        np.testing.assert_array_equal(r2[own], r[own])
    np.testing.assert_array_equal(total, whole[0])
    if kind == "int":
        np.testing.assert_array_equal(whole[0], A.ranks(S, seen, answers)[0])
        # a part that owns no answer
        lo, Ep = parts[-1]
        a0 = np.zeros(B, np.int64)
        r, v = rank_range(ht, Ep, seen, a0, base=lo, answer_score=np.zeros(B, np.float32))
        np.testing.assert_array_equal(r, A.ranks(S, seen, a0, lo, lo + Ep.shape[0], answer_score=np.zeros(B, np.float32))[0])
        untouched = score_range(ht, Ep, seen, a0, lo, torch.full((B,), 5.0, device="cuda"))
        assert (untouched == 5.0).all()


def test_graph_capture_replays_with_new_inputs():
    L, lib = _lib()
    rng = np.random.default_rng(6)
    B, V, d = 130, 4099, 64
    h = torch.from_numpy(rng.standard_normal((B, d)).astype(np.float32)).cuda()
    E = torch.from_numpy(rng.standard_normal((V, d)).astype(np.float32)).cuda()
    seen = [rng.choice(V, size=30, replace=False).tolist() for _ in range(B)]
    indptr, indices = csr_of(seen)
    users = torch.arange(B, device="cuda")
    ans = torch.from_numpy(rng.integers(0, V, size=B)).cuda()
    rank = torch.empty(B, dtype=torch.int32, device="cuda")
    val = torch.empty(B, dtype=torch.float32, device="cuda")
    s = torch.cuda.Stream()

    def call(stream):
        L.check(lib.bsarec_answer_rank(h.data_ptr(), d, E.data_ptr(), B, V, d, users.data_ptr(), indptr.data_ptr(),
                                       indices.data_ptr(), ans.data_ptr(), rank.data_ptr(), val.data_ptr(), stream.cuda_stream),
                "bsarec_answer_rank")
    with torch.cuda.stream(s):
        call(s)                                          # eager warm-up
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    with torch.cuda.stream(s):
        call(s)
    torch.cuda.synchronize()
    assert torch.cuda.max_memory_allocated() == before   # no allocation
    first = rank.cpu().numpy().copy()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        call(s)
    torch.cuda.synchronize()
    h.copy_(torch.from_numpy(rng.standard_normal((B, d)).astype(np.float32)))
    ans.copy_(torch.from_numpy(rng.integers(0, V, size=B)))
    g.replay()
    torch.cuda.synchronize()
    got = (rank.cpu().numpy().copy(), val.cpu().numpy().copy())
    assert (got[0] != first).any()
    assert_same(got, rank_range(h, E, seen, ans.cpu().numpy(), entry="whole"))
    g.replay()                                           # and again: the same ranks (the launch starts from its own correction)
    torch.cuda.synchronize()
    np.testing.assert_array_equal(rank.cpu().numpy(), got[0])


def test_trainer_rank_mode_on_a_tiny_model():
    """eval_full_rank = "rank" against the dense mode through Trainer.iteration: the six reference values and the extras to
    1e-12, the same '{:.4f}' strings, and the MRR key."""
    import scipy.sparse as sp
    from bsarec_amd import BSARecModel
    from bsarec_amd.trainer import Trainer
    from test_gpu_boundary import ns
    rng = np.random.default_rng(2)
    V, n, Lq = 97, 150, 50
    a = ns(item_size=V, extra_ks=(1, 50))
    torch.manual_seed(1)
    model = BSARecModel(a).cuda()
    model.eval()
    ids = rng.integers(1, V, size=(n, Lq))
    ids[np.arange(Lq)[None, :] < rng.integers(0, Lq - 2, size=n)[:, None]] = 0
    answers = rng.integers(1, V, size=n)
    rows = np.repeat(np.arange(n), 12)
    cols = rng.integers(1, V, size=n * 12)
    a.train_matrix = sp.csr_matrix((np.ones(len(cols)), (rows, cols)), shape=(n, V))
    batches = [(torch.arange(i, min(n, i + 64)), torch.from_numpy(ids[i:i + 64]), torch.from_numpy(answers[i:i + 64]),
                torch.zeros(1), torch.zeros(1)) for i in range(0, n, 64)]
    tr = Trainer(model, None, None, None, a, None)
    dense, dline = tr.iteration(3, batches, train=False)
    a.eval_full_rank = "rank"
    got, gline = tr.iteration(3, batches, train=False)
    assert len(dense) == 10 and len(got) == 11
    np.testing.assert_allclose(got[:10], dense, rtol=0, atol=1e-12)
    assert gline.startswith(dline[:-1]) and gline[len(dline) - 1:] == f", 'MRR': '{got[10]:.4f}'}}"
    ranks = torch.cat([tr.answer_ranks(u.cuda(), x.cuda(), y.cuda()) for u, x, y, _, _ in batches]).cpu().numpy()
    assert got[10] == pytest.approx(float(np.mean(1.0 / (ranks + 1.0))), abs=1e-15)
    deep, line = tr.get_rank_score(0, ranks, extra_ks=(V,))
    assert deep[6] == 1.0 and "'HR@97': '1.0000'" in line


def test_shipped_checkpoint_metrics_in_rank_mode():
    """The shipped LastFM checkpoint's logged test metrics, through Trainer.iteration with eval_full_rank = "rank"."""
    from test_gpu_full_rank import _kat_trainer
    from bsarec_amd import data as D
    from test_gpu_boundary import load_kat
    z, tr, ins = _kat_trainer("LastFM", eval_full_rank="rank")
    _, cfg, seqs = load_kat("LastFM")
    users, ins, ans = D.eval_table(seqs, 50, "test")
    batches = [(torch.from_numpy(users[i:i + 256]), torch.from_numpy(ins[i:i + 256]), torch.from_numpy(ans[i:i + 256]),
                torch.zeros(1), torch.zeros(1)) for i in range(0, len(users), 256)]
    vals, line = tr.iteration(0, batches, train=False)
    np.testing.assert_allclose(vals[:6], z["metrics"], rtol=0, atol=1e-12)
    assert len(vals) == 7 and 0 < vals[6] < 1 and "'MRR'" in line and f"'HR@10': '{z['metrics'][2]:.4f}'" in line
