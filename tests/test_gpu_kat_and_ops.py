"""GPU tests beyond the e2e goldens: the reference's shipped checkpoints as known-answer tests through
the HIP eval path, per-op FrequencyLayer vectors, a full-size C1 step against the oracle, the Trainer
loop (graph replay == eager), and size-independent properties at the bench's full size."""
import argparse
import ctypes as C
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, load_e2e, rel_l2

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")


def ns(**kw):
    a = argparse.Namespace(item_size=97, hidden_size=64, max_seq_length=50, batch_size=256, hidden_dropout_prob=0.5,
                           attention_probs_dropout_prob=0.5, num_hidden_layers=2, num_attention_heads=2,
                           hidden_act="gelu", initializer_range=0.02, c=3, alpha=0.9, seed=42, lr=1e-3,
                           adam_beta1=0.9, adam_beta2=0.999, weight_decay=0.0, no_cuda=False, log_freq=1)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def load_kat(name):
    z = np.load(os.path.join(GOLDEN, f"kat_{name}.npz"))
    cfg = json.loads(str(z["cfg"]))
    off, items = z["seq_offsets"], z["seq_items"]
    seqs = [items[off[i]:off[i + 1]].tolist() for i in range(len(off) - 1)]
    return z, cfg, seqs


@pytest.mark.parametrize("name", ["LastFM", "Beauty"])
def test_shipped_checkpoint_known_answers(name):
    """src/output/BSARec_{name}_best.pt through BSARecModel + Trainer.test on the GPU reproduces the
    reference's six logged test metrics, its top-10 lists and its logits."""
    import scipy.sparse as sp
    from bsarec_amd import BSARecModel, data as D
    from bsarec_amd.trainer import Trainer
    z, cfg, seqs = load_kat(name)
    a = ns(item_size=cfg["item_size"], num_attention_heads=cfg["num_attention_heads"], c=cfg["c"], alpha=cfg["alpha"])
    model = BSARecModel(a)
    model.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p/")})
    model = model.cuda()
    users, ins, ans = D.eval_table(seqs, 50, "test")
    test_dl = D.DeviceBatches(users, ins, ans, 256, "cuda", shuffle=False)
    indptr, cols = D.seen_csr(seqs, "test")
    a.test_rating_matrix = sp.csr_matrix((np.ones(len(cols)), cols, indptr), shape=(len(seqs), cfg["item_size"]))
    a.valid_rating_matrix = a.test_rating_matrix
    tr = Trainer(model, None, None, test_dl, a, None)
    scores, info = tr.test(0)
    np.testing.assert_allclose(scores, z["metrics"], rtol=0, atol=1e-12)
    model.eval()
    logits = model.full_logits(torch.from_numpy(ins[:8]).cuda()).cpu().numpy()
    assert np.abs(logits - z["logits8"]).max() <= 1e-3 * np.abs(z["logits8"]).max()
    assert np.abs(logits - z["logits8"]).max() <= 5e-5
    # formatted like the reference log line
    assert f"'HR@10': '{z['metrics'][2]:.4f}'" in info and f"'NDCG@10': '{z['metrics'][3]:.4f}'" in info


def test_frequency_layer_op_vs_reference_vectors():
    """Stand-alone FrequencyLayer entry points vs the imported reference for 8 (L, c) combos incl.
    c >= L, odd L and L = 7."""
    from bsarec_amd import _lib
    from bsarec_amd.model import _twiddle
    lib = _lib.load()
    z = np.load(os.path.join(GOLDEN, "freq_ops.npz"))
    st = torch.cuda.current_stream().cuda_stream
    for i, (L, c) in enumerate(z["combos"]):
        L, c = int(L), int(c)
        cb = min(c // 2 + 1, L // 2 + 1)
        t = {k: torch.from_numpy(z[f"{i}/{k}"]).cuda().contiguous() for k in ("x", "gy", "sqrt_beta", "ln_w", "ln_b")}
        B, _, d = t["x"].shape
        tw = _twiddle(L).cuda()
        y, xhat = torch.empty_like(t["x"]), torch.empty_like(t["x"])
        rstd = torch.empty(B * L, device="cuda")
        rc = lib.bsarec_freq_layer_fwd(t["x"].data_ptr(), t["sqrt_beta"].data_ptr(), t["ln_w"].data_ptr(),
                                       t["ln_b"].data_ptr(), tw.data_ptr(), B, L, d, cb, 1e-12, 0.0, None, 0,
                                       y.data_ptr(), xhat.data_ptr(), rstd.data_ptr(), st)
        assert rc == 0
        np.testing.assert_allclose(y.cpu().numpy(), z[f"{i}/y"], atol=5e-6)
        scratch = torch.empty(lib.bsarec_freq_layer_bwd_scratch_floats(B, L, d), device="cuda")
        dx = torch.empty_like(t["x"])
        dsb, dlw, dlb = (torch.empty(d, device="cuda") for _ in range(3))
        rc = lib.bsarec_freq_layer_bwd(t["x"].data_ptr(), t["gy"].data_ptr(), xhat.data_ptr(), rstd.data_ptr(),
                                       t["sqrt_beta"].data_ptr(), t["ln_w"].data_ptr(), tw.data_ptr(), B, L, d, cb, 0.0,
                                       None, 0, scratch.data_ptr(), dx.data_ptr(), dsb.data_ptr(), dlw.data_ptr(),
                                       dlb.data_ptr(), st)
        assert rc == 0
        torch.cuda.synchronize()
        np.testing.assert_allclose(dx.cpu().numpy(), z[f"{i}/dx"], atol=3e-5)
        np.testing.assert_allclose(dsb.cpu().numpy(), z[f"{i}/dsqrt_beta"].reshape(-1), rtol=2e-4, atol=3e-5)
        np.testing.assert_allclose(dlw.cpu().numpy(), z[f"{i}/dln_w"], rtol=2e-4, atol=2e-5)
        np.testing.assert_allclose(dlb.cpu().numpy(), z[f"{i}/dln_b"], rtol=2e-4, atol=2e-5)


def _c1_model_and_batch(B=256, V=3417, seed=0):
    from bsarec_amd import BSARecModel, data as D
    torch.manual_seed(seed)
    model = BSARecModel(ns(item_size=V)).cuda()
    seqs = D.synth_ml1m_like(seed=1, n_users=400, n_items=V - 1)
    u, x, a = D.train_table(seqs, 50)
    rng = np.random.default_rng(seed)
    pick = rng.permutation(len(a))[:B]
    return model, x[pick], a[pick]


def test_full_size_c1_training_step_vs_oracle():
    """The bench's own configuration (B=256, L=50, d=64, V=3417, 2 layers, dropout 0.5): loss, logits and
    all gradients of one step against the oracle (same Philox masks)."""
    from oracle import bsarec_oracle as O
    model, ids, ans = _c1_model_and_batch()
    model.train()
    model.set_seed(7)
    params = {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()}
    loss = model.calculate_loss(torch.from_numpy(ids).cuda(), torch.from_numpy(ans).cuda(), None, None, None)
    loss.backward()
    cfg = O.Config(item_size=3417)
    oloss, ologits, G, _ = O.loss_and_grads(params, cfg, ids, ans, O.DropoutSpec(True, 7, 1))
    assert abs(loss.item() - oloss) <= 5e-6 * abs(oloss)
    from bsarec_amd import _lib as Lb
    logits = model._plan(256).view(Lb.BUF_LOGITS, 0, (256, 3420))[:, :3417].cpu().numpy()
    assert np.abs(logits - ologits).max() <= 1e-3 * np.abs(ologits).max()
    for k, g in model.grad_views().items():
        if k.endswith("key.bias"):
            assert g.abs().max().item() <= 1e-6
            continue
        assert rel_l2(g.cpu().numpy(), G[k]) <= 2e-4, (k, rel_l2(g.cpu().numpy(), G[k]))


def test_full_size_properties_batch_equivariance_and_normalisation():
    """Size-independent properties at the bench size: eval outputs are per-sequence (permuting the batch
    permutes the outputs bit for bit), attention rows sum to 1, per-row dlogits sum to 0."""
    from bsarec_amd import _lib as Lb
    model, ids, ans = _c1_model_and_batch()
    model.eval()
    t = torch.from_numpy(ids).cuda()
    perm = torch.randperm(256, device="cuda")
    a = model.forward(t).detach()
    b = model.forward(t[perm]).detach()
    assert torch.equal(a[perm], b)
    plan = model._plan(256)
    probs = plan.view(Lb.BUF_PROBS, 0, (256, 2, 50, 52))
    np.testing.assert_allclose(probs.sum(-1).cpu().numpy(), 1.0, atol=2e-6)
    assert probs[..., 50:].abs().max().item() == 0
    x = a.cpu().numpy()                                    # LN output with gamma=1, beta=0 at init
    np.testing.assert_allclose(x.mean(-1), 0, atol=1e-5)
    np.testing.assert_allclose(x.var(-1), 1, atol=1e-3)


def test_trainer_loop_graph_replay_equals_eager_and_learns():
    """Trainer.iteration(train=True): hipGraph replay (incl. several steps per graph launch) and eager launches give the
    same parameters (same Philox stream, deterministic reductions; the tolerance below dates from the float-atomic scatter), the
    short last batch goes through its own plan, and the loss goes down."""
    from bsarec_amd import BSARecModel, data as D
    from bsarec_amd.trainer import Trainer
    seqs = D.synth_ml1m_like(seed=3, n_users=60, n_items=300)
    u, x, a = D.train_table(seqs, 50)
    u, x, a = u[:1100], x[:1100], a[:1100]                  # 4 full batches + a short one
    res = {}
    for mode in ("graph", "eager"):
        torch.manual_seed(1)
        model = BSARecModel(ns(item_size=301)).cuda()
        model.set_seed(5)
        dl = D.DeviceBatches(u, x, a, 256, "cuda", shuffle=True, seed=11)
        tr = Trainer(model, dl, None, None, ns(item_size=301), None, use_graph=(mode == "graph"))
        tr.steps_per_graph = 2                  # 4 full batches per epoch: pairs of steps replay as ONE graph launch
        losses = [float(tr.train(e)["rec_loss"]) for e in range(3)]
        if mode == "graph":
            assert any(k[0] == "indexed_multi" for k in tr._graphs if isinstance(k, tuple)), "multi-step graph not exercised"
        res[mode] = (losses, {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()})
        assert losses[-1] < losses[0]
    # (tolerance from when the embedding scatter used float atomics -- last-bit differences in dE, which Adam turns into a
    #  +-lr step where the gradient is ~0 -- kept: compare up to a tiny fraction of such elements)
    np.testing.assert_allclose(res["graph"][0], res["eager"][0], atol=2e-4)
    for k in res["graph"][1]:
        bad = np.abs(res["graph"][1][k] - res["eager"][1][k]) > 2e-5
        assert bad.mean() <= 2e-3, (k, bad.mean())


def test_config3_shape_generic_path_vs_oracle():
    """BASELINE config 3 shape (L=200, hidden=256, 4 heads, 4 layers) at a small batch: generic tiled kernels
    (256-wide LayerNorm / softmax tiles, 4 layers of ping-pong gradients) against the oracle, dropout on."""
    from oracle import bsarec_oracle as O
    from bsarec_amd import BSARecModel
    cfg = O.Config(item_size=301, hidden_size=256, max_seq_length=200, num_hidden_layers=4, num_attention_heads=4, c=9,
                   alpha=0.7, hidden_dropout_prob=0.3, attention_probs_dropout_prob=0.2)
    params = O.init_params(cfg, seed=3)
    rng = np.random.default_rng(3)
    B, L = 3, 200
    ids = np.zeros((B, L), dtype=np.int64)
    for b, n in enumerate((200, 37, 0)):
        if n:
            ids[b, L - n:] = rng.integers(1, 301, size=n)
    ans = rng.integers(1, 301, size=B).astype(np.int64)
    a = ns(item_size=301, hidden_size=256, max_seq_length=200, num_hidden_layers=4, num_attention_heads=4, c=9, alpha=0.7,
           hidden_dropout_prob=0.3, attention_probs_dropout_prob=0.2)
    model = BSARecModel(a)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params.items()})
    model = model.cuda()
    model.train()
    model.set_seed(11)
    loss = model.calculate_loss(torch.from_numpy(ids).cuda(), torch.from_numpy(ans).cuda(), None, None, None)
    loss.backward()
    oloss, _, G, _ = O.loss_and_grads(params, cfg, ids, ans, O.DropoutSpec(True, 11, 1))
    assert abs(loss.item() - oloss) <= 1e-5 * abs(oloss)
    for k, g in model.grad_views().items():
        if k.endswith("key.bias"):
            continue
        assert rel_l2(g.cpu().numpy(), G[k]) <= 3e-4, (k, rel_l2(g.cpu().numpy(), G[k]))


def test_config4_shape_large_batch_and_catalogue_runs_and_learns():
    """BASELINE config 4 shape per GPU (V=20034, 1024 sequences per step): the fused step runs, stays finite and
    the loss decreases; the short last batch and hipGraph replay are exercised at this size too."""
    from bsarec_amd import BSARecModel, data as D
    from bsarec_amd.trainer import Trainer
    seqs = D.synth_ml1m_like(seed=5, n_users=200, n_items=20033)
    u, x, a_ = D.train_table(seqs, 50)
    u, x, a_ = u[:2500], x[:2500], a_[:2500]
    torch.manual_seed(0)
    a = ns(item_size=20034)
    model = BSARecModel(a).cuda()
    dl = D.DeviceBatches(u, x, a_, 1024, "cuda", shuffle=True, seed=1)
    tr = Trainer(model, dl, None, None, a, None)
    losses = [float(tr.train(e)["rec_loss"]) for e in range(4)]
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


@pytest.mark.parametrize("shape", ["d64_L50_N1", "C5_d256_L256_N2"])
def test_config5_scale_catalogue_ten_million_items_properties(shape):
    """BASELINE config 5's catalogue (V = 10,000,001; logits rows of 40 MB, B*V > 2^31 elements) through the same
    entry points -- at the fused shape class (d = 64, L = 50, 1 layer) and at C5's OWN shape (L = 256,
    hidden 256, 4 heads, 2 layers, B = 256: generic tiled kernels, a 10.24 GB fp32 table with 41 GB of parameter +
    gradient + Adam state, 10 GB logits rows streamed by the CE kernel): the loss equals a float64 log-sum-exp recomputed
    from the encoder output in catalogue chunks, every dlogits row sums to zero (so do the untouched-by-lookup columns of
    dE), sampled dE rows equal dlogits^T . h_last, and one Adam step moves exactly the rows that received gradient.
    Size-independent properties only: the numpy oracle does not run at this size."""
    from bsarec_amd import BSARecModel, _lib as Lb
    V, B = 10_000_001, 256
    Lq, d, N, heads = (50, 64, 1, 2) if shape == "d64_L50_N1" else (256, 256, 2, 4)
    a = ns(item_size=V, num_hidden_layers=N, hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, hidden_size=d,
           max_seq_length=Lq, num_attention_heads=heads)
    torch.manual_seed(3)
    model = BSARecModel(a).cuda()
    model.train()
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    ids = torch.randint(1, V, (B, Lq), device="cuda", generator=g)
    ids[:, :20][torch.rand(B, 20, device="cuda", generator=g) < 0.5] = 0
    ids[:, :20] = torch.where(torch.cummin(ids[:, :20].flip(1), 1).values.flip(1) == 0, 0, ids[:, :20])   # left padding
    ans = torch.randint(1, V, (B,), device="cuda", generator=g)
    ans[:4] = torch.tensor([1, V - 1, V - 2, 5_000_000], device="cuda")         # catalogue edges
    loss = model.calculate_loss(ids, ans)
    loss.backward()
    with torch.no_grad():
        h = model.forward(ids)[:, -1, :].double()                                # dropout off: same activations
    E = model.item_embeddings.weight.detach()
    m = torch.full((B,), -1e30, dtype=torch.float64, device="cuda"); ssum = torch.zeros_like(m)
    for v0 in range(0, V, 1_000_000):
        lg = h @ E[v0:v0 + 1_000_000].double().T
        m2 = torch.maximum(m, lg.max(1).values)
        ssum = ssum * torch.exp(m - m2) + torch.exp(lg - m2[:, None]).sum(1)
        m = m2
    lse = m + torch.log(ssum)
    tgt = (h * E[ans].double()).sum(1)
    ref = float((lse - tgt).mean().item())
    assert abs(loss.item() - ref) <= 2e-6 * abs(ref), (loss.item(), ref)
    plan = model._plan(B)
    Vp = (V + 3) // 4 * 4
    dlog = plan.view(Lb.BUF_DLOGITS, 0, (B, Vp))
    assert float(dlog.double().sum(1).abs().max().item()) <= 1e-6
    assert float(dlog[:, V:].abs().max().item()) == 0.0
    dE = model.item_embeddings.weight.grad
    probe = torch.tensor([0, 7, 123_457, 4_999_999, 9_999_999, V - 1], device="cuda")
    probe = probe[~torch.isin(probe, ids.flatten())]                              # rows without a lookup gradient
    want = dlog[:, probe].double().T @ h
    assert float((dE[probe].double() - want).abs().max().item()) <= 2e-5 * float(want.abs().max().item())   # fp32 sum over 256 rows
    # lookup rows: dE[row] - logits part = sum of the embedding-path gradient rows of that id (non-zero for used ids)
    used = torch.unique(ids[ids > 0])[:64]
    lookup = dE[used].double() - dlog[:, used].double().T @ h
    assert float(lookup.abs().sum(1).min().item()) > 0.0
    before = E[probe].clone()
    model.configure_adam(lr=1e-3)
    model.adam_step()
    moved = (model.item_embeddings.weight.detach()[probe] - before).abs().max(1).values
    assert bool((moved > 0).all())                       # every catalogue row has a (tiny) softmax gradient
    assert torch.isfinite(model.item_embeddings.weight.detach()).all()


def test_data_parallel_step_one_rank_rccl_equals_single_gpu_step():
    """The data-parallel step (forward / backward, summing all-reduce of the flat gradient arena over RCCL,
    Adam on sum / world) on a 1-rank "nccl" group gives the same parameters as the fused single-GPU step."""
    import socket
    import torch.distributed as dist
    from bsarec_amd import BSARecModel, data as D
    from bsarec_amd.trainer import Trainer
    s = socket.socket(); s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]; s.close()
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1,
                            device_id=torch.device("cuda", 0))
    try:
        seqs = D.synth_ml1m_like(seed=3, n_users=40, n_items=300)
        u, x, a_ = D.train_table(seqs, 50)
        u, x, a_ = u[:768], x[:768], a_[:768]
        res = {}
        for mode in ("single", "dp", "dp_graph", "dp_graph2"):
            torch.manual_seed(1)
            model = BSARecModel(ns(item_size=301)).cuda()
            model.set_seed(5)
            dl = D.DeviceBatches(u, x, a_, 256, "cuda", shuffle=True, seed=11)
            tr = Trainer(model, dl, None, None, ns(item_size=301), None, use_graph=mode.startswith("dp_graph"),
                         process_group=dist.group.WORLD if mode != "single" else None)
            tr.dp_graph = "two" if mode == "dp_graph2" else "one"
            losses = [float(tr.train(e)["rec_loss"]) for e in range(2)]
            res[mode] = (losses, {k: v.detach().cpu().numpy().copy() for k, v in model.state_dict().items()})
            if mode == "dp_graph":
                assert tr.dp_graph == "one", "capture of the RCCL all-reduce inside the step graph was refused"
        # "dp_graph": ONE graph with the RCCL all-reduce captured inside; "dp_graph2": graph A + eager all-reduce + graph B
        for mode in ("dp", "dp_graph", "dp_graph2"):
            np.testing.assert_allclose(res["single"][0], res[mode][0], atol=2e-4)
            for k in res["single"][1]:
                bad = np.abs(res["single"][1][k] - res[mode][1][k]) > 2e-5
                assert bad.mean() <= 2e-3, (k, bad.mean())
    finally:
        dist.destroy_process_group()


def test_train_from_scratch_lastfm_follows_the_reference_log():
    """End to end on real data: train LastFM from scratch with the reference's hyper-parameters through the
    reference-style driver (early stopping on NDCG@20, best parameters reloaded, test metrics).  Random streams
    differ from the authors' run, so the comparison is statistical: the epoch losses follow the shipped log
    (src/output/BSARec_LastFM_best.log:61, :121, :211 -> 7.9817, 5.3795, 4.8757) and the test metrics land in
    the band of the logged ones (:237 -> HR@10 0.0807, NDCG@10 0.0435; 1,090 test users)."""
    import logging
    from bsarec_amd import main as M
    z, cfg, seqs = load_kat("LastFM")
    losses = []

    class Grab(logging.Handler):
        def emit(self, rec):
            m = str(rec.getMessage())
            if "rec_loss" in m:
                losses.append(float(m.split("'rec_loss': '")[1].split("'")[0]))
    logger = logging.getLogger("bsarec_test_train")
    logger.setLevel(logging.INFO)
    logger.addHandler(Grab())
    args = M.parse_args(["--data_name", "LastFM", "--lr", "0.001", "--num_attention_heads", "1", "--c", "3", "--alpha", "0.9"])
    scores, info, epochs, secs = M.run(args, seqs, logger)
    assert abs(losses[0] - 7.9817) < 0.08 and abs(losses[20] - 5.3795) < 0.15, (losses[0], losses[20])
    assert epochs >= 25 and losses[-1] < 5.2
    ref = z["metrics"]
    assert 0.6 * ref[2] <= scores[2] <= 1.4 * ref[2], (scores, ref)          # HR@10
    assert 0.7 * ref[3] <= scores[3] <= 1.3 * ref[3], (scores, ref)          # NDCG@10


def test_tiled_weight_gradient_fallback_matches_too():
    """cfg.dw_tiled = 1 (LDS-tiled grouped weight-gradient kernel at the fused shape, instead of the direct one) is a
    per-plan option: the dropout-on oracle parity case (loss + all gradients, pruned and full top block) must pass
    through it as well, in this process, next to plans that use the direct kernel."""
    from bsarec_amd import _lib as Lb
    import test_gpu_parity as P
    try:
        for prune in (1, 0):
            Lb.set_default_options(dw_tiled=1, no_prune_top=1 - prune)
            P._dropout_training_step_vs_oracle("A_d64_L50_h2", 37, prune)
    finally:
        Lb.set_default_options(dw_tiled=0, no_prune_top=0)
