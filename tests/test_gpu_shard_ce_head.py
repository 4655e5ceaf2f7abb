"""The range form of the full-catalogue CE head on the GPU (bsarec_ce_head_range_stats / _merge / _bwd) and the catalogue-sharded
step that uses it (ShardedCatalogue with shard_ce_head = "fused"): one range over the whole table against bsarec_ce_head_fwd /
_bwd bit for bit, W ranges held by one process against the fp64 restatement (shard_ce_head_ref), determinism, graph replay, two
and three ranks on one GPU against ONE model on the global batch, peak memory, and the whole step replayed from one graph."""
import os
import socket
import time

import numpy as np
import pytest

from conftest import rel_l2
import shard_ce_head_ref as SR

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")
G = 0.37


def _inputs(Bg, V, d):
    """fp32-rounded h [Bg, d] ~ N(0, 1) and E [V, d] ~ N(0, 1 / d), as tests/test_gpu_ce_head.py draws them."""
    rng = np.random.default_rng(100003 * Bg + 101 * V + d)
    return rng, rng.normal(0, 1, (Bg, d)).astype(np.float32), rng.normal(0, 1 / np.sqrt(d), (V, d)).astype(np.float32)


def _gpu(*arrays):
    return [torch.from_numpy(np.ascontiguousarray(x)).cuda() for x in arrays]


class Rank:
    """One range [lo, lo + vs) of E in this process: its rows, workspace and outputs (NaN-filled before every call)."""

    def __init__(self, h, E, a, lo, vs, V, g=G):
        from bsarec_amd import _lib
        self.L, self.lib = _lib, _lib.load()
        self.h, self.a, self.lo, self.vs, self.V = h, a, lo, vs, V
        self.Bg, self.d = h.shape
        self.rows = E[lo:lo + vs].clone() if vs else torch.zeros(1, self.d, device="cuda")
        self.nb = self.lib.bsarec_ce_head_range_workspace_bytes(self.Bg, vs, self.d)
        assert 0 < self.nb <= (16384 + 2 * self.Bg) * (self.d + 8) * 4
        self.ws = torch.zeros(self.nb, dtype=torch.uint8, device="cuda")
        self.stats = torch.full((3, self.Bg), float("nan"), device="cuda")
        self.loss, self.loss_rows = torch.full((1,), float("nan"), device="cuda"), torch.full((self.Bg,), float("nan"), device="cuda")
        self.dh = torch.full((self.Bg, self.d), float("nan"), device="cuda")
        self.dE = torch.full((max(vs, 1), self.d), float("nan"), device="cuda")
        self.g = torch.full((1,), g, device="cuda")

    def run_stats(self):
        st = torch.cuda.current_stream().cuda_stream
        self.L.check(self.lib.bsarec_ce_head_range_stats(self.h.data_ptr(), self.h.stride(0), self.rows.data_ptr(), self.Bg, self.vs,
                                                         self.lo, self.V, self.d, self.a.data_ptr(), self.stats.data_ptr(),
                                                         self.ws.data_ptr(), self.nb, st), "bsarec_ce_head_range_stats")

    def run_merge_bwd(self, stats_all):
        st = torch.cuda.current_stream().cuda_stream
        self.L.check(self.lib.bsarec_ce_head_range_merge(stats_all.data_ptr(), stats_all.shape[0], self.Bg, self.ws.data_ptr(), self.nb,
                                                         self.loss_rows.data_ptr(), self.loss.data_ptr(), st),
                     "bsarec_ce_head_range_merge")
        self.L.check(self.lib.bsarec_ce_head_range_bwd(self.h.data_ptr(), self.h.stride(0), self.rows.data_ptr(), self.Bg, self.vs,
                                                       self.lo, self.V, self.d, self.a.data_ptr(), self.g.data_ptr(),
                                                       self.ws.data_ptr(), self.nb, self.dh.data_ptr(), self.dE.data_ptr(), st),
                     "bsarec_ce_head_range_bwd")


def _sharded(h, E, a, W):
    """The W ranges through stats -> (the gather) -> merge -> bwd, all in this process: the ranks and stats_all."""
    V = E.shape[0]
    ranks = [Rank(h, E, a, lo, vs, V) for lo, vs in SR.ranges(V, W)]
    for r in ranks:
        r.run_stats()
    stats_all = torch.stack([r.stats for r in ranks]).contiguous()
    for r in ranks:
        r.run_merge_bwd(stats_all)
    torch.cuda.synchronize()
    return ranks, stats_all


# ---- one range over the whole table ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,V,d", [(33, 1000, 64), (65, 4099, 160), (33, 129, 256)])
def test_one_range_over_the_whole_table_is_the_single_table_head_bit_for_bit(B, V, d):
    from bsarec_amd import _lib
    lib = _lib.load()
    rng, h, E = _inputs(B, V, d)
    a = rng.integers(-2, V + 2, B).astype(np.int64)
    a[:4] = [0, V - 1, -3, V + 5]
    h, E, a = _gpu(h, E, a)
    nb = lib.bsarec_ce_head_workspace_bytes(B, V, d)
    assert nb == lib.bsarec_ce_head_range_workspace_bytes(B, V, d)
    ws = torch.zeros(nb, dtype=torch.uint8, device="cuda")
    loss, rows = torch.full((1,), float("nan"), device="cuda"), torch.full((B,), float("nan"), device="cuda")
    dh, dE = torch.full((B, d), float("nan"), device="cuda"), torch.full((V, d), float("nan"), device="cuda")
    gout = torch.full((1,), G, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.bsarec_ce_head_fwd(h.data_ptr(), d, E.data_ptr(), B, V, d, a.data_ptr(), loss.data_ptr(), rows.data_ptr(),
                                      ws.data_ptr(), nb, st), "bsarec_ce_head_fwd")
    _lib.check(lib.bsarec_ce_head_bwd(h.data_ptr(), d, E.data_ptr(), B, V, d, a.data_ptr(), gout.data_ptr(), ws.data_ptr(), nb,
                                      dh.data_ptr(), dE.data_ptr(), st), "bsarec_ce_head_bwd")
    (r,), _ = _sharded(h, E, a, 1)
    assert (r.lo, r.vs) == (0, V)
    for name, got, want in (("loss", r.loss, loss), ("rows", r.loss_rows, rows), ("dh", r.dh, dh), ("dE", r.dE, dE)):
        assert torch.isfinite(want).all(), name
        assert torch.equal(got, want), name
    assert float(dh.abs().max()) > 0 and float(dE.abs().max()) > 0


# ---- W ranges in one process against fp64 ------------------------------------------------------------------------------------
def _forced_answers(V, W):
    """One id shared by two rows, -3 and V + 5 (the clamp brings them in range), id 0, V - 1, every shard's first and last row."""
    s = V // 2
    ends = [x for lo, vs in SR.ranges(V, W) if vs for x in (lo, lo + vs - 1)]
    return [s, s, -3, V + 5, 0, V - 1] + sorted(set(ends))


# (300, 4099, 64, 2): the boundary at row 2050 is no multiple of 128, several row tiles; (130, 70001, 160, 3): several splits,
# ce_dh_kernel<1, 8>; (8, 5, 64, 8): three ranks own nothing
SHARDED = [(96, 301, 64, 2), (40, 1000, 128, 3), (16, 37, 64, 8), (8, 5, 64, 8), (300, 4099, 64, 2), (130, 70001, 160, 3)]


@pytest.mark.parametrize("Bg,V,d,W", SHARDED)
def test_ranges_in_one_process_against_the_fp64_restatement(Bg, V, d, W):
    """Gates of test_kernel_vs_fp64_reference: loss 5e-6 rel, rows 1e-5 abs, the sum of the dh parts 1e-4 rel-L2, the
    concatenated dE 1e-4 rel-L2 over the table and over the rows that are nobody's answer.  The forced answers go in as many
    answer vectors of Bg rows as they need (two at (16, 37, 64, 8) and at (8, 5, 64, 8))."""
    rng, h, E = _inputs(Bg, V, d)
    cut = SR.ranges(V, W)
    if (Bg, V, W) == (8, 5, 8):
        assert [vs for _, vs in cut] == [1, 1, 1, 1, 1, 0, 0, 0]
    if (V, W) == (4099, 2):
        assert cut[1][0] == 2050
    forced = _forced_answers(V, W)
    th, tE = _gpu(h, E)
    for at in range(0, len(forced), Bg):
        a = rng.integers(0, V, Bg).astype(np.int64)
        part = forced[at:at + Bg]
        a[:len(part)] = part
        want_loss, want_rows, want_dh, want_dE, want_stats = SR.sharded_ce_head(h, E, a, W, G)
        ranks, stats_all = _sharded(th, tE, _gpu(a)[0], W)
        for r, st in zip(ranks, want_stats):                                  # the exchanged statistics themselves
            got = r.stats.cpu().numpy().astype(np.float64)
            if r.vs == 0:
                assert (got[0] == -np.inf).all() and not got[1:].any()
                assert not r.dh.any().item() and torch.isnan(r.dE).all()      # dh_part zeroed, nothing else touched
                continue
            assert np.array_equal(got[2] != 0, st[2] != 0)                    # the owner, and only the owner, wrote the target
            assert np.abs(got[0] - st[0]).max() <= 1e-5 and np.abs(got[2] - st[2]).max() <= 1e-5
        for r in ranks[1:]:                                                    # every rank merged the same bits
            assert torch.equal(r.loss, ranks[0].loss) and torch.equal(r.loss_rows, ranks[0].loss_rows)
        loss, rows = ranks[0].loss.item(), ranks[0].loss_rows.cpu().numpy().astype(np.float64)
        dh = sum(r.dh.cpu().numpy().astype(np.float64) for r in ranks)
        dE = np.concatenate([r.dE[:r.vs].cpu().numpy() for r in ranks])
        assert dE.shape == (V, d) and np.isfinite(dh).all() and np.isfinite(dE).all()
        rest = np.ones(V, bool)
        rest[SR.clamp(a, V)] = False
        e_loss, e_rows = abs(loss - want_loss) / abs(want_loss), np.abs(rows - want_rows).max()
        e_dh, e_dE = rel_l2(dh, sum(want_dh)), rel_l2(dE, np.concatenate(want_dE))
        e_rest = rel_l2(dE[rest], np.concatenate(want_dE)[rest]) if rest.any() else 0.0
        print(f"range ce_head Bg={Bg} V={V} d={d} W={W} answers {at}..: loss {loss:.7f} rel {e_loss:.2e} rows {e_rows:.2e} "
              f"dh {e_dh:.2e} dE {e_dE:.2e} dE(non-answer rows) {e_rest:.2e}")
        assert e_loss <= 5e-6
        assert e_rows <= 1e-5
        assert e_dh <= 1e-4
        assert e_dE <= 1e-4 and e_rest <= 1e-4


# ---- determinism, graph replay ----------------------------------------------------------------------------------------------
def test_two_calls_agree_and_a_graph_replays_the_eager_call():
    """Rank 1 of 2 (column base 2050, no multiple of 128) at (300, 4099, 64): two eager calls give equal bits; stats + merge + bwd
    captured once (the gather left out: the other rank's statistics sit in stats_all) and replayed after h, E and g were
    overwritten in place equal the eager call on the new values."""
    Bg, V, d, W = 300, 4099, 64, 2
    rng, h, E = _inputs(Bg, V, d)
    a = rng.integers(0, V, Bg).astype(np.int64)
    a[:8] = _forced_answers(V, W)[:8]
    h, E, a = _gpu(h, E, a)
    first, stats_all = _sharded(h, E, a, W)
    second, stats_again = _sharded(h, E, a, W)
    assert torch.equal(stats_all, stats_again)
    for p, q in zip(first, second):
        for name in ("loss", "loss_rows", "dh", "dE"):
            assert torch.equal(getattr(p, name), getattr(q, name)), name
    (lo, vs) = SR.ranges(V, W)[1]
    assert lo == 2050
    r = Rank(h, E, a, lo, vs, V, g=1.0)
    sall = stats_all.clone()

    def step():
        r.run_stats()
        sall[1].copy_(r.stats)
        r.run_merge_bwd(sall)

    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        step()                                                # first launches (kernel attributes) outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=s):
        step()
    torch.cuda.synchronize()
    gen = torch.Generator(device="cuda").manual_seed(9)
    h.copy_(torch.randn(Bg, d, device="cuda", generator=gen))
    E.copy_(torch.randn(V, d, device="cuda", generator=gen) / 8)
    r.rows.copy_(E[lo:lo + vs])
    r.g.fill_(G)
    want, want_stats = _sharded(h, E, a, W)
    sall[0].copy_(want_stats[0])                              # what the gather would bring from rank 0
    for t in (r.loss, r.loss_rows, r.dh, r.dE):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    for name in ("stats", "loss", "loss_rows", "dh", "dE"):
        assert torch.equal(getattr(r, name), getattr(want[1], name)), name
    assert float(r.dh.abs().max()) > 0 and float(r.dE.abs().max()) > 0


# ---- ranks -------------------------------------------------------------------------------------------------------------------
def _spawn(fn, world, *args, limit=240):
    """One process per rank (at most 3 plus this one); the ranks are ended when ``limit`` seconds have passed."""
    import torch.multiprocessing as mp
    assert world <= 3
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    ctx = mp.spawn(fn, args=(world, port) + args, nprocs=world, join=False)
    deadline = time.monotonic() + limit
    while not ctx.join(timeout=5):
        if time.monotonic() > deadline:
            for p in ctx.processes:
                p.kill()
            pytest.fail(f"{fn.__name__}: the ranks did not finish within {limit} s")


def _worker(rank, world, port, kw, out_dir):
    import torch.distributed as dist
    from bsarec_amd.catalogue import ShardedCatalogue
    from test_gpu_catalogue_shard import _batches, _full_model, _ns, _seen
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        ns = _ns(shard_ce_head="fused", eval_full_rank="fused", **kw)
        B = ns.batch_size
        sc = ShardedCatalogue(ns, B, dist.group.WORLD, "cuda:0")
        assert sc.ce_head == "fused" and sc.logits is None and not hasattr(sc, "scratch")
        sc.load_full_state_dict(_full_model(ns).state_dict())
        mine = slice(rank * B, (rank + 1) * B)
        losses = [float(sc.train_step(ids[mine], ans[mine])) for ids, ans in _batches(ns, 3, world * B)]
        assert not sc.px.timed_out()
        ids, _ = _batches(ns, 1, world * B)[0]
        sc.topk(ids[mine], 20, _seen(ns, world * B)[mine])
        assert sc.logits is None                                      # neither the step nor the evaluation allocated it
        sd = {k: v.detach().cpu().numpy() for k, v in sc.full_state_dict().items()}
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), losses=np.asarray(losses), **sd)
        sc.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,kw", [(2, dict()), (2, dict(hidden_size=128, max_seq_length=64, num_attention_heads=4, item_size=1003, c=9)),
                                      (3, dict(item_size=302, batch_size=16))],
                         ids=["W2_fused_d64_L50", "W2_generic_d128_L64", "W3_uneven_shards"])
def test_ranks_fused_ce_head_equals_the_full_table_step(world, kw, tmp_path):
    """The three configurations of test_ranks_sharded_catalogue_equals_the_full_table_step with shard_ce_head = "fused" (gloo,
    real hipIpc), three steps: replicas and gathered tables bit-identical across ranks; losses and every parameter against ONE
    BSARecModel on the global batch at that test's gates."""
    from test_gpu_catalogue_shard import _batches, _full_model, _ns
    _spawn(_worker, world, kw, str(tmp_path))
    r0 = np.load(tmp_path / "rank0.npz")
    for r in range(1, world):
        rr = np.load(tmp_path / f"rank{r}.npz")
        for k in r0.files:
            np.testing.assert_array_equal(r0[k], rr[k], err_msg=k)
    ns = _ns(**kw)
    model = _full_model(ns)
    model.configure_adam(lr=ns.lr, betas=(ns.adam_beta1, ns.adam_beta2), weight_decay=ns.weight_decay)
    model.train()
    losses = [float(model.train_step(ids.cuda(), ans.cuda())) for ids, ans in _batches(ns, 3, world * ns.batch_size)]
    print(f"fused sharded CE, W={world}: losses {r0['losses']} one model {losses}")
    np.testing.assert_allclose(r0["losses"], losses, atol=2e-4)
    sd = model.state_dict()
    assert set(sd) == set(r0.files) - {"losses"}
    for k in sd:
        got, want = r0[k], sd[k].detach().cpu().numpy()
        assert got.shape == want.shape, k
        bad = np.abs(got - want) > 2e-5
        assert bad.mean() <= 2e-3, (k, bad.mean(), np.abs(got - want).max())


def _memory_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    from bsarec_amd.catalogue import ShardedCatalogue
    from test_gpu_catalogue_shard import _batches, _ns, _seen
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        ns = _ns(item_size=400_001, batch_size=16, shard_ce_head="fused", eval_full_rank="fused")
        B = ns.batch_size
        sc = ShardedCatalogue(ns, B, dist.group.WORLD, "cuda:0")
        matrix = sc.Bg * sc.Vs * 4
        assert matrix == 32 * (200_001, 200_000)[rank] * 4
        assert sc.logits is None and not hasattr(sc, "scratch")
        mine = slice(rank * B, (rank + 1) * B)
        ids, ans = _batches(ns, 1, world * B)[0]
        seen = _seen(ns, world * B)[mine]

        def step_and_topk():
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            held = torch.cuda.memory_allocated()
            loss = float(sc.train_step(ids[mine], ans[mine]))
            sc.topk(ids[mine], 20, seen)
            torch.cuda.synchronize()
            return loss, torch.cuda.max_memory_allocated() - held

        # the first step and evaluation create what every head creates once: the encoder's plans, the evaluation's workspace
        _, first = step_and_topk()
        # what the object holds by now: no tensor but the shard, its gradient and its moments reaches a quarter of the matrix
        held_big = {k: v.numel() * v.element_size() for k, v in vars(sc).items()
                    if torch.is_tensor(v) and v.numel() * v.element_size() >= matrix // 4}
        assert set(held_big) <= {"E", "dE", "m", "v"}, held_big
        loss, grown = step_and_topk()
        print(f"rank {rank}: [Bg, Vs] fp32 {matrix} B, CE workspace {sc.ce_ws_bytes} B, step + topk peak above what is held: "
              f"first {first} B, then {grown} B")
        assert np.isfinite(loss) and sc.logits is None
        assert grown < matrix // 4, (grown, matrix)
        np.savez(os.path.join(out_dir, f"mem{rank}.npz"), grown=grown, matrix=matrix, ws=sc.ce_ws_bytes)
        sc.close()
    finally:
        dist.destroy_process_group()


def test_fused_step_and_fused_evaluation_never_hold_a_bg_by_vs_matrix(tmp_path):
    """W = 2, 400,001 items, d = 64, B = 16: a [Bg, Vs] fp32 matrix is 25.6 MB per rank.  The object holds no tensor of a quarter
    of that besides the shard, its gradient and its two moments (51 MB each, whatever the head), and one training step plus
    one top-k raise torch.cuda.max_memory_allocated by less than that quarter above what is held when they start.  Measured on
    the second step and evaluation: the first ones create the encoder's plans and the evaluation's workspace, which every head
    creates once and keeps (their peak is printed).  A condition, not a measurement: the step allocates small operands only."""
    _spawn(_memory_worker, 2, str(tmp_path))
    for r in range(2):
        m = np.load(tmp_path / f"mem{r}.npz")
        assert 0 < int(m["ws"]) < int(m["matrix"]) // 4 and int(m["grown"]) < int(m["matrix"]) // 4


def _graph_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    from bsarec_amd.catalogue import ShardedCatalogue
    from test_gpu_catalogue_shard import _batches, _ns
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world,
                            device_id=torch.device("cuda", 0))
    try:
        ns = _ns(hidden_dropout_prob=0.3, attention_probs_dropout_prob=0.2, shard_ce_head="fused", eval_full_rank="fused")
        B = ns.batch_size
        res = {}
        for mode in ("eager", "graph"):
            torch.manual_seed(7)                                     # the encoder replica draws its weights from torch's generator
            sc = ShardedCatalogue(ns, B, dist.group.WORLD, "cuda:0")
            losses = []
            for ids, ans in _batches(ns, 4, B):
                step = sc.train_step_graph if mode == "graph" else sc.train_step
                losses.append(float(step(ids.cuda(), ans.cuda()).item()))
            if mode == "graph":
                assert sc.graph_captured, getattr(sc, "_graph_error", "no capture attempted")
            assert sc.logits is None
            sc.check_exchange()
            res[mode] = (losses, {k: v.detach().cpu().numpy() for k, v in sc.full_state_dict().items()})
            sc.close()
        np.savez(os.path.join(out_dir, "graph.npz"), le=np.asarray(res["eager"][0]), lg=np.asarray(res["graph"][0]),
                 **{"e/" + k: v for k, v in res["eager"][1].items()}, **{"g/" + k: v for k, v in res["graph"][1].items()})
    finally:
        dist.destroy_process_group()


def test_fused_sharded_step_replays_from_one_graph_rccl_one_rank(tmp_path):
    """ShardedCatalogue.train_step_graph with shard_ce_head = "fused" in a 1-rank RCCL group: the captured step equals its eager
    twin (same dropout stream), at the gates of the dense step's graph test."""
    _spawn(_graph_worker, 1, str(tmp_path))
    z = np.load(tmp_path / "graph.npz")
    np.testing.assert_allclose(z["lg"], z["le"], rtol=1e-5)
    for k in [k[2:] for k in z.files if k.startswith("e/")]:
        a, b = z["g/" + k], z["e/" + k]
        bad = np.abs(a - b) > 2e-5
        assert bad.mean() <= 2e-3, (k, bad.mean(), np.abs(a - b).max())
