"""ShardedCatalogue.full_sort_scores(full_rank="rank"): two and three ranks on one GPU (gloo control plane, hipIpc mappings).
The metrics from the summed per-shard answer ranks equal those of full_rank="fused" (lists, candidate gathers, merge), with
repeated ids in the ``seen`` argument and with a catalogue the ranks do not divide evenly; the ranks themselves equal
bsarec_answer_rank on the gathered table, exactly."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def _seen_with_repeats(ns, Bg):
    from test_gpu_catalogue_shard import _seen
    seen = _seen(ns, Bg)
    return torch.cat([seen, seen[:, :6], seen[:, 3:4].expand(-1, 3)], 1).contiguous()      # ids two and five times, pads between


def _worker(rank, world, port, kw, out_dir):
    import torch.distributed as dist
    from bsarec_amd.catalogue import ShardedCatalogue
    from test_gpu_catalogue_shard import _batches, _full_model, _ns
    torch.cuda.set_device(0)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world)
    try:
        ns = _ns(**kw)
        B = ns.batch_size
        sc = ShardedCatalogue(ns, B, dist.group.WORLD, "cuda:0")
        sc.load_full_state_dict(_full_model(ns).state_dict())
        for ids, ans in _batches(ns, 2, world * B):
            sc.train_step(ids[rank * B:(rank + 1) * B], ans[rank * B:(rank + 1) * B])
        ids, _ = _batches(ns, 1, world * B)[0]
        seen = _seen_with_repeats(ns, world * B)
        mine = slice(rank * B, (rank + 1) * B)
        fv, fi = sc.topk(ids[mine], 20, seen[mine], full_rank="fused")
        # answers: list positions 0, 3, 12 and 19, an item the row has seen, and items outside every list
        pos = torch.tensor([0, 3, 12, 19], device=fi.device)[torch.arange(B, device=fi.device) % 4]
        ans = torch.gather(fi, 1, pos.view(-1, 1)).view(-1)
        ans[5] = seen[mine][5, 2].to(ans.device)
        ans[6::8] = torch.arange(1, ns.item_size, 37, device=ans.device)[:len(ans[6::8])]
        batch = [(ids[mine], ans, seen[mine]), (ids[mine], torch.flip(ans, (0,)), None)]
        fused, ftxt = sc.full_sort_scores(batch, epoch=2, extra_ks=(1, 15), full_rank="fused")
        ranked, rtxt = sc.full_sort_scores(batch, epoch=2, extra_ks=(1, 15), full_rank="rank")
        r = sc.answer_ranks(ids[mine], ans, seen[mine])
        torch.cuda.synchronize()
        h_all, ans_all = sc.h_all.cpu().numpy().copy(), sc.ans_all.cpu().numpy().copy()
        sc.args.eval_full_rank = "rank"                                # the flag: full_sort_scores takes it, topk refuses it
        flagged, _ = sc.full_sort_scores(batch, epoch=2, extra_ks=(1, 15))
        with pytest.raises(ValueError, match="produces no lists"):
            sc.topk(ids[mine], 20, seen[mine])
        deep, _ = sc.full_sort_scores(batch[:1], extra_ks=(ns.item_size,))        # deeper than any list
        sd = {k: v.detach().cpu().numpy() for k, v in sc.full_state_dict().items()}
        np.savez(os.path.join(out_dir, f"rank{rank}.npz"), fused=np.asarray(fused), ranked=np.asarray(ranked),
                 flagged=np.asarray(flagged), deep=np.asarray(deep), same_text=np.asarray(ftxt == rtxt), r=r.cpu().numpy(),
                 h_all=h_all, ans_all=ans_all, E=sd["item_embeddings.weight"], fi=fi.cpu().numpy(), ans=ans.cpu().numpy())
        sc.close()
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,kw", [(2, dict()), (3, dict(item_size=302, batch_size=16))], ids=["W2_uneven", "W3_uneven_shards"])
def test_rank_mode_metrics_equal_the_fused_mode(world, kw, tmp_path):
    """(W2: 301 rows = 151 + 150; W3: 302 rows = 101 + 101 + 100.)"""
    from bsarec_amd import ranking
    from test_gpu_catalogue_shard import _ns
    from test_gpu_shard_full_rank import _spawn
    _spawn(_worker, world, kw, str(tmp_path))
    z = [np.load(tmp_path / f"rank{r}.npz") for r in range(world)]
    ns = _ns(**kw)
    B = ns.batch_size
    assert ns.item_size % world != 0
    for r in range(world):
        np.testing.assert_allclose(z[r]["ranked"], z[r]["fused"], rtol=0, atol=1e-12)
        np.testing.assert_array_equal(z[r]["flagged"], z[r]["ranked"])
        np.testing.assert_array_equal(z[r]["ranked"], z[0]["ranked"])              # every rank: the GLOBAL numbers
        assert bool(z[r]["same_text"]) and z[r]["deep"][6] == 1.0
    assert 0 < z[0]["ranked"][0] < z[0]["ranked"][4] < 1                           # hits and misses at the cutoffs
    # the ranks: bsarec_answer_rank on the gathered table, and the positions the answers were taken from
    h, E = torch.from_numpy(z[0]["h_all"]).cuda(), torch.from_numpy(z[0]["E"]).cuda()
    seen = _seen_with_repeats(ns, world * B).cuda()
    S = seen.shape[1]
    users = torch.arange(world * B, device="cuda")
    csr = (torch.arange(world * B + 1, device="cuda") * S, seen)
    want = ranking.answer_rank(h, E, torch.from_numpy(z[0]["ans_all"]).cuda(), users, csr).cpu().numpy()
    for r in range(world):
        rows = slice(r * B, (r + 1) * B)
        np.testing.assert_array_equal(z[r]["ans_all"][rows], z[r]["ans"])
        np.testing.assert_array_equal(z[r]["r"], want[rows], err_msg=f"rank {r}")
        for b in range(B):
            where = np.nonzero(z[r]["fi"][b] == z[r]["ans"][b])[0]
            assert (where.size == 1 and where[0] == z[r]["r"][b]) or (where.size == 0 and z[r]["r"][b] >= 20)
