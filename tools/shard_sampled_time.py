"""ms per step of ONE rank of the catalogue-sharded step (bsarec_amd/catalogue.py) with the full-catalogue CE head, the
sampled-softmax head (train_negatives = N) and lazy Adam for the shard (train_lazy_adam), plus peak memory.  A 1-rank
RCCL group (as the graph test): the step replays from one hipGraph.  One configuration per process, so that a caller can
give each its own time limit:

    python tools/shard_sampled_time.py --Vs 1250001                    # full-catalogue CE
    python tools/shard_sampled_time.py --Vs 1250001 --neg 8192         # sampled head, dense Adam over the shard
    python tools/shard_sampled_time.py --Vs 1250001 --neg 8192 --lazy  # sampled head, lazy Adam

Default shape: one C5 shard -- 1,250,001 owned rows, d = 256, 2,048 sequences (the Bg of a C5 rank's
full-CE head), L = 50, 2 layers, 4 heads, dropout 0.1.  Prints one JSON line."""
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
    ap.add_argument("--neg", type=int, default=0, help="0: full-catalogue CE, else the sampled head's N")
    ap.add_argument("--lazy", action="store_true", help="lazy Adam for the shard (needs --neg > 0)")
    ap.add_argument("--popularity", action="store_true", help="popularity sampler (default uniform)")
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
        ns = argparse.Namespace(item_size=a.Vs, hidden_size=a.hidden, max_seq_length=L, batch_size=B, hidden_dropout_prob=0.1,
                                attention_probs_dropout_prob=0.1, num_hidden_layers=2, num_attention_heads=4, hidden_act="gelu",
                                initializer_range=0.02, c=5, alpha=0.7, seed=42, lr=1e-3, adam_beta1=0.9, adam_beta2=0.999,
                                weight_decay=0.0, train_negatives=a.neg, train_lazy_adam=a.lazy,
                                train_sampler="popularity" if a.popularity else "uniform")
        sc = ShardedCatalogue(ns, B, dist.group.WORLD, "cuda:0")
        rng = np.random.default_rng(0)
        if a.popularity:
            sc.set_train_popularity(np.maximum(1, (1e6 / np.arange(1, a.Vs + 1) ** 0.8)).astype(np.int64))
        ids = torch.from_numpy(rng.integers(1, a.Vs, size=(B, L)).astype(np.int64)).cuda()
        ans = torch.from_numpy(rng.integers(1, a.Vs, size=B).astype(np.int64)).cuda()
        for _ in range(a.warmup):
            sc.train_step_graph(ids, ans)
        torch.cuda.synchronize()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(a.steps):
            loss = sc.train_step_graph(ids, ans)
        t1.record()
        torch.cuda.synchronize()
        step_ms = t0.elapsed_time(t1) / a.steps
        assert np.isfinite(float(loss)), float(loss)
        free, total = torch.cuda.mem_get_info()
        sc.check_exchange()
        print(json.dumps({"Vs": a.Vs, "d": a.hidden, "batch": B, "neg": a.neg, "lazy": a.lazy, "popularity": a.popularity,
                          "graph": sc.graph_captured, "ms_per_step": round(step_ms, 3), "loss": round(float(loss), 5),
                          "torch_peak_gb": round(torch.cuda.max_memory_allocated() / 2**30, 2),
                          "device_used_gb": round((total - free) / 2**30, 2)}), flush=True)
        sc.close()
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
