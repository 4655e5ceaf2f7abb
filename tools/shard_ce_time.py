"""ms per step and peak memory of ONE rank of the catalogue-sharded full-CE step (bsarec_amd/catalogue.py) with the dense head
(partial logits [Bg, Vs]) and with the fused head (shard_ce_head = "fused": no [Bg, Vs] buffer).  A 1-rank
RCCL group as in tools/shard_sampled_time.py; both steps replay from their own hipGraph in one process and alternate call by
call, a hipEvent pair around each replay:

    python tools/shard_ce_time.py --Vs 1250001
    python tools/shard_ce_time.py --Vs 125001

Default shape: one C5 shard -- 1,250,001 owned rows, d = 256, 2,048 sequences, L = 50, 2 layers, 4 heads, dropout
0.1.  The peaks are per head: the growth of torch.cuda.max_memory_allocated and of the device's used memory from before the
object is built to after its warm-up steps (the fused object is built first; the caching allocator keeps what it has).
Prints one JSON line."""
import argparse
import json
import os
import socket
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--Vs", type=int, default=1_250_001, help="owned rows (= the catalogue: one rank)")
    ap.add_argument("--batch", type=int, default=2048)
    ap.add_argument("--hidden", type=int, default=256)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    import torch.distributed as dist
    from bsarec_amd.catalogue import ShardedCatalogue
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        B, L = a.batch, 50
        rng = np.random.default_rng(0)
        ids = torch.from_numpy(rng.integers(1, a.Vs, size=(B, L)).astype(np.int64)).cuda()
        ans = torch.from_numpy(rng.integers(1, a.Vs, size=B).astype(np.int64)).cuda()
        heads, out = {}, {"Vs": a.Vs, "d": a.hidden, "batch": B, "steps": a.steps}
        for head in ("fused", "dense"):
            ns = argparse.Namespace(item_size=a.Vs, hidden_size=a.hidden, max_seq_length=L, batch_size=B, hidden_dropout_prob=0.1,
                                    attention_probs_dropout_prob=0.1, num_hidden_layers=2, num_attention_heads=4,
                                    hidden_act="gelu", initializer_range=0.02, c=5, alpha=0.7, seed=42, lr=1e-3, adam_beta1=0.9,
                                    adam_beta2=0.999, weight_decay=0.0, shard_ce_head=head, eval_full_rank="fused")
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            held, free0 = torch.cuda.memory_allocated(), torch.cuda.mem_get_info()[0]
            sc = ShardedCatalogue(ns, B, dist.group.WORLD, "cuda:0")
            for _ in range(a.warmup):
                loss = sc.train_step_graph(ids, ans)
            torch.cuda.synchronize()
            assert sc.graph_captured, getattr(sc, "_graph_error", "no capture attempted")
            assert (sc.logits is None) == (head == "fused")
            heads[head] = sc
            out[head] = {"loss": round(float(loss), 5),
                         "torch_peak_mb": round((torch.cuda.max_memory_allocated() - held) / 2**20, 1),
                         "device_used_mb": round((free0 - torch.cuda.mem_get_info()[0]) / 2**20, 1)}
        ms = {head: [] for head in heads}
        for _ in range(a.steps):
            for head, sc in heads.items():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                loss = sc.train_step_graph(ids, ans)
                t1.record()
                torch.cuda.synchronize()
                ms[head].append(t0.elapsed_time(t1))
                assert np.isfinite(float(loss)), (head, float(loss))
        for head, sc in heads.items():
            t = np.asarray(ms[head])
            out[head].update(ms_median=round(float(np.median(t)), 3), ms_min=round(float(t.min()), 3), ms_max=round(float(t.max()), 3))
            sc.check_exchange()
        print(json.dumps(out), flush=True)
        for sc in heads.values():
            sc.close()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
