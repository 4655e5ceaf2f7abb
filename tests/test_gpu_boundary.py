"""Bit-exact / boundary GPU tests (VERDICT r1 "close the bit-exact gaps"):

* the device-side batch assembly of the indexed training step against plain indexing of the sample table
  (index work: equality, not a tolerance) -- src/dataset.py:207-211 (RandomSampler + collation);
* the GPU top-20 lists of the shipped checkpoints against the reference's (src/trainers.py:134-149);
* Trainer.save -> Trainer.load and `--do_eval` through the reference-flag driver (src/trainers.py:43-60, src/main.py:37-45);
* the reference's own optimisation loop -- calculate_loss / zero_grad / backward / torch.optim.Adam.step over
  model.parameters() (src/trainers.py:27-28,103-107) -- against the reference's parameters after three steps;
* the dropout step counter across the eager tail batch of an epoch.
"""
import argparse
import json
import os

import numpy as np
import pytest

from conftest import E2E_CASES, GOLDEN, ROOT, load_e2e

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


@pytest.mark.parametrize("variant", ["in_block", "separate_embed", "generic"])
def test_indexed_step_assembles_exactly_the_indexed_batch(variant):
    """After every bsarec_train_step_indexed the plan's id / answer buffers must equal inputs[perm[c : c + B]] /
    answers[perm[c : c + B]] exactly and the device cursor must have advanced by B -- through the bottom block's phase 0
    (fused path), the stand-alone embedding kernel, and the generic path; the last step straddles the end of the
    permutation (rows past n read sample perm-independent row 0, as the header states)."""
    from bsarec_amd import BSARecModel, _lib as Lb
    V, L, B = 211, 50, 64
    rng = np.random.default_rng(5)
    n = 3 * B + 17
    inputs = rng.integers(0, V, size=(n, L)).astype(np.int64)
    inputs[rng.random((n, L)) < 0.4] = 0
    answers = rng.integers(1, V, size=n).astype(np.int64)
    opts = {"in_block": {}, "separate_embed": dict(separate_embed=1), "generic": dict(no_fused=1)}[variant]
    old = Lb.set_default_options(**opts) if opts else {}
    try:
        m = BSARecModel(ns(item_size=V)).cuda()
        m.train()
        m.configure_adam()
        table, ans_t = torch.from_numpy(inputs).cuda(), torch.from_numpy(answers).cuda()
        perm = torch.from_numpy(rng.permutation(n).astype(np.int64)).cuda()
        cursor = torch.zeros(1, dtype=torch.int64, device="cuda")
        for step in range(4):
            c = step * B
            loss = m.train_step_indexed(table, ans_t, perm, cursor, B)
            plan = m._plan(B)
            src = torch.where(torch.arange(c, c + B, device="cuda") < n,
                              perm[torch.arange(c, c + B, device="cuda").clamp(max=n - 1)], torch.zeros((), dtype=torch.int64, device="cuda"))
            assert torch.equal(plan.ids_buf, table[src]), (variant, step)
            assert torch.equal(plan.ans_buf, ans_t[src]), (variant, step)
            assert int(cursor.item()) == c + B
            assert np.isfinite(loss.item())
    finally:
        if old:
            Lb.set_default_options(**old)


def test_gather_batch_entry_point_is_exact():
    """bsarec_gather_batch alone (the C entry a host without the fused step would call)."""
    from bsarec_amd import _lib as Lb
    lib = Lb.load()
    rng = np.random.default_rng(11)
    n, L, B = 1000, 50, 256
    table = torch.from_numpy(rng.integers(0, 5000, size=(n, L)).astype(np.int64)).cuda()
    ans = torch.from_numpy(rng.integers(1, 5000, size=n).astype(np.int64)).cuda()
    perm = torch.from_numpy(rng.permutation(n).astype(np.int64)).cuda()
    ids_out = torch.zeros((B, L), dtype=torch.int64, device="cuda")
    ans_out = torch.zeros(B, dtype=torch.int64, device="cuda")
    for c in (0, 256, 700, 744):
        cursor = torch.tensor([c], dtype=torch.int64, device="cuda")
        Lb.check(lib.bsarec_gather_batch(table.data_ptr(), ans.data_ptr(), perm.data_ptr(), n, cursor.data_ptr(), B, L,
                                         ids_out.data_ptr(), ans_out.data_ptr(), torch.cuda.current_stream().cuda_stream), "gather")
        k = min(B, n - c)
        assert torch.equal(ids_out[:k], table[perm[c:c + k]])
        assert torch.equal(ans_out[:k], ans[perm[c:c + k]])
        if k < B:                                            # past the end: sample 0
            assert torch.equal(ids_out[k:], table[0].expand(B - k, L))


@pytest.mark.parametrize("name", ["LastFM", "Beauty"])
def test_shipped_checkpoint_top20_lists(name):
    """The GPU eval path's top-20 id lists (seen items := 0, src/trainers.py:134-149) of the first 64 test users equal
    the reference's lists.  Index work: exact.  Where two candidates are closer than fp32 noise in score (the fixture
    compares CPU torch with this GPU path) a swap is accepted only if the GPU scores of the two items differ by less
    than 2e-5 -- none is expected."""
    import scipy.sparse as sp
    from bsarec_amd import BSARecModel, data as D
    from bsarec_amd.trainer import Trainer
    z, cfg, seqs = load_kat(name)
    a = ns(item_size=cfg["item_size"], num_attention_heads=cfg["num_attention_heads"], c=cfg["c"], alpha=cfg["alpha"])
    model = BSARecModel(a)
    model.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p/")})
    model = model.cuda()
    model.eval()
    users, ins, ans = D.eval_table(seqs, 50, "test")
    indptr, cols = D.seen_csr(seqs, "test")
    a.test_rating_matrix = sp.csr_matrix((np.ones(len(cols)), cols, indptr), shape=(len(seqs), cfg["item_size"]))
    a.valid_rating_matrix = a.test_rating_matrix
    a.train_matrix = a.test_rating_matrix
    tr = Trainer(model, None, None, None, a, None)
    pred, scores = tr.topk_after_seen(torch.arange(64, device="cuda"), torch.from_numpy(ins[:64]).cuda(), return_scores=True)
    pred = pred.cpu().numpy()
    want = z["top20_64"].astype(np.int64)
    if not np.array_equal(pred, want):
        sc = scores.cpu().numpy()
        for u, r in zip(*np.nonzero(pred != want)):
            assert abs(sc[u, pred[u, r]] - sc[u, want[u, r]]) < 2e-5, (u, r, pred[u], want[u])
        assert (pred != want).mean() < 0.01
    np.testing.assert_array_equal(pred[:, :10], want[:, :10])


def test_trainer_save_load_round_trip_and_do_eval_cli(tmp_path):
    """Trainer.save writes the reference's 42-key state_dict; Trainer.load of that file restores every tensor bit for
    bit; and `python -m bsarec_amd.main --do_eval --load_model X` (src/main.py:37-45) reproduces the shipped
    checkpoint's logged LastFM test metrics from the file Trainer.save wrote."""
    from bsarec_amd import BSARecModel, data as D, main as M
    from bsarec_amd.trainer import Trainer
    from bsarec_amd.model import param_shapes
    z, cfg, seqs = load_kat("LastFM")
    a = ns(item_size=cfg["item_size"], num_attention_heads=cfg["num_attention_heads"], c=cfg["c"], alpha=cfg["alpha"])
    model = BSARecModel(a)
    model.load_state_dict({k[2:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("p/")})
    tr = Trainer(model.cuda(), None, None, None, a, None)
    path = str(tmp_path / "BSARec_LastFM_rt.pt")
    tr.save(path)
    sd = torch.load(path, map_location="cpu", weights_only=True)
    assert list(sd.keys()) == list(param_shapes(a).keys()) and len(sd) == 42
    torch.manual_seed(1)
    other = BSARecModel(a)                                         # different random init
    tr2 = Trainer(other.cuda(), None, None, None, a, None)
    tr2.load(path)
    for k, v in tr2.model.state_dict().items():
        assert torch.equal(v.cpu(), torch.from_numpy(z["p/" + k])), k
    # the CLI: data file in the reference's txt format, checkpoint under output_dir
    D.write_user_seqs(str(tmp_path / "LastFM.txt"), seqs)
    res = M.main(["--data_dir", str(tmp_path) + "/", "--data_name", "LastFM", "--output_dir", str(tmp_path) + "/",
                  "--do_eval", "--load_model", "BSARec_LastFM_rt", "--train_name", "rt_eval",
                  "--num_attention_heads", str(cfg["num_attention_heads"]), "--c", str(cfg["c"]), "--alpha", str(cfg["alpha"])])
    scores, info = res[0], res[1]
    np.testing.assert_allclose(scores, z["metrics"], rtol=0, atol=1e-12)
    assert f"'HR@10': '{z['metrics'][2]:.4f}'" in info
    assert os.path.exists(tmp_path / "rt_eval.log")
    # --do_eval without --load_model: logs and returns (src/main.py:38-40)
    assert M.main(["--data_dir", str(tmp_path) + "/", "--data_name", "LastFM", "--output_dir", str(tmp_path) + "/", "--do_eval",
                   "--train_name", "rt_none"]) is None


@pytest.mark.parametrize("name", E2E_CASES[:3])
def test_reference_style_loop_with_torch_adam(name):
    """the reference Trainer's own loop -- loss = model.calculate_loss(...); optim.zero_grad();
    loss.backward(); optim.step() with torch.optim.Adam over model.parameters() (arena views) -- three steps against the
    reference's parameters after three steps (fixture a/, dropout 0)."""
    from test_gpu_parity import build_model
    cfg, params, _, after, z = load_e2e(name)
    model = build_model(cfg, params)
    model.train()
    optim = torch.optim.Adam(model.parameters(), lr=1e-3, betas=(0.9, 0.999), weight_decay=0.0)     # src/trainers.py:27-28
    ids = torch.from_numpy(z["ids"]).cuda()
    ans = torch.from_numpy(z["answers"]).cuda()
    losses = []
    for _ in range(3):
        loss = model.calculate_loss(ids, ans, None, None, None)
        optim.zero_grad()
        loss.backward()
        optim.step()
        losses.append(loss.item())
    np.testing.assert_allclose(losses, z["adam_losses"], rtol=5e-6)
    arena0 = model._arena.data_ptr()
    sd = model.state_dict()
    for k, a in after.items():
        got = sd[k].cpu().numpy()
        if k.endswith("key.bias"):
            assert np.abs(got - a).max() <= 3.5e-3
            continue
        bad = np.abs(got - a) > 2e-5
        assert bad.mean() <= 2e-3, (k, bad.mean(), np.abs(got - a).max())
    # the optimiser updated the arena in place: parameters are still views of it
    assert model._arena.data_ptr() == arena0
    p0 = next(model.parameters())
    assert p0.data_ptr() == model._arena.data_ptr()


def test_dropout_step_counter_is_never_reused_across_the_epoch_tail():
    """An epoch of the Trainer = full batches as indexed graph replays + one eager tail batch.  The indexed step uses the
    dropout step counter as it stands and advances it at its end; the eager step advances it first.  Every optimisation
    step must see its own counter value (the tail step and the next epoch's first step drew the same masks)."""
    from bsarec_amd import BSARecModel, data as D
    from bsarec_amd.trainer import Trainer
    V, L, B = 97, 50, 32
    rng = np.random.default_rng(3)
    n = 3 * B + 5
    inputs = rng.integers(1, V, size=(n, L)).astype(np.int64)
    answers = rng.integers(1, V, size=n).astype(np.int64)
    a = ns(item_size=V, batch_size=B)
    dl = D.DeviceBatches(np.arange(n), inputs, answers, B, "cuda", shuffle=True, seed=1)
    model = BSARecModel(a).cuda()
    tr = Trainer(model, dl, None, None, a, None)
    used = []
    orig_idx, orig_eager = tr.indexed_step, tr._step_eager

    def spy_idx(*x, **k):
        r = orig_idx(*x, **k)
        s = int(model._state[1].item())                    # a group of _last_multi steps replays as one graph launch:
        used.extend(range(s - tr._last_multi, s))         # each used the value before its closing increment
        return r

    def spy_eager(*x, **k):
        r = orig_eager(*x, **k)
        used.append(int(model._state[1].item()))           # incremented first, then used
        return r
    tr.indexed_step, tr._step_eager = spy_idx, spy_eager
    for ep in range(3):
        tr.train(ep)
    assert len(used) == 3 * 4
    assert all(b > a for a, b in zip(used, used[1:])), used


def test_bench_command_of_the_driver_builds_no_graph_on_the_clock():
    """`python bench.py --gpus 1 --steps 20 --warmup 5` (the driver's command, BENCH_r02.json): every graph of the run is
    built by Feed.prepare() before t0 (timed_steps asserts it), 20 steps = a 16-step and a 4-step graph launch, and the
    result equals 20 eager steps from the same state (same Philox stream, same batches)."""
    import bench
    from bsarec_amd import BSARecModel, data as D
    from bsarec_amd.trainer import Trainer, graph_sizes
    a = argparse.Namespace(item_size=301, hidden=64, seq_len=50, batch=32, layers=2, heads=2, dtype="f32")
    margs = bench.model_args(a)
    seqs = D.synth_ml1m_like(seed=3, n_users=200, n_items=300)
    u, x, y = D.train_table(seqs, 50)

    def run(graph):
        torch.manual_seed(0)
        model = BSARecModel(margs).cuda()
        model.set_seed(9)
        model.train()
        bt = D.DeviceBatches(u, x, y, 32, "cuda", shuffle=True, seed=4)
        tr = Trainer(model, bt, None, None, margs, None, use_graph=graph)
        fd = bench.Feed(tr, bt, "cuda")
        dt, loss = bench.timed_steps(fd, 20, 5, torch.cuda.synchronize)
        return tr, fd, float(loss.item()), model._arena.clone()
    tr, fd, loss_g, arena_g = run(True)
    assert tr.graphs_built() == len(graph_sizes(16))
    ran = fd.pos // 32
    tr2, fd2, loss_e, arena_e = run(False)
    # the eager run took fewer untimed steps (no graphs to build): bring it to the same step count before comparing
    assert fd2.pos // 32 == 25 and ran > 25
    fd2.run(ran - 25)
    torch.cuda.synchronize()
    # (a tolerance from when the embedding scatter summed with float atomics: Adam turns a sign flip of a ~0 gradient into
    #  a +-lr step -- compare up to a small fraction of such elements, as the graph-vs-eager test does)
    bad = (arena_g - tr2.model._arena).abs() > 5e-5
    print("graph vs eager after", ran, "steps: fraction off", bad.float().mean().item())
    assert bad.float().mean().item() <= 1e-2


def test_bench_dump_outputs_of_the_last_timed_step(tmp_path):
    """`bench.py --steps K --dump-outputs DIR`, run twice with the same arguments: the result line counts exactly K timed steps
    and holds ms_per_step; DIR holds the last step's loss and the parameters after its Adam update (the state_dict keys) in
    float32.  Same inputs and a step without order-dependent float sums: the two runs write the same bits -- also when the
    second one goes on to the roofline section, whose extra eager steps on the same model must come after the dump."""
    import subprocess
    import sys
    from bsarec_amd import BSARecModel
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "2", "--batch", "32",
           "--item_size", "301", "--no-secondary", "--no-cpu-baseline"]
    lines = []
    for i, extra in enumerate((["--no-roofline"], [])):
        r = subprocess.run(cmd + extra + ["--dump-outputs", str(tmp_path / f"run{i}")], capture_output=True, text=True,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        lines.append(json.loads(r.stdout.strip().splitlines()[-1]))
    for line in lines:
        assert line["steps"] == 7 and line["ms_per_step"] > 0
        assert line["dump_outputs"]["sampled"] == [] and line["dump_outputs"]["bytes"] <= 64 << 20
    assert "roofline" not in lines[0] and "roofline" in lines[1]
    import bench
    a = argparse.Namespace(item_size=301, hidden=64, seq_len=50, batch=32, layers=2, heads=2, dtype="f32")
    params = BSARecModel(bench.model_args(a)).state_dict()
    assert sorted(os.listdir(tmp_path / "run0")) == sorted([f"{k}.npy" for k in params] + ["loss.npy"])
    l0, l1 = (np.load(tmp_path / f"run{i}" / "loss.npy") for i in range(2))
    assert l0.dtype == np.float32 and l0.shape == (1,)
    assert all(abs(float(l0[0]) - line["config"]["final_loss"]) <= 1e-4 for line in lines)
    assert np.array_equal(l0, l1)
    for k, t in params.items():
        p0, p1 = (np.load(tmp_path / f"run{i}" / f"{k}.npy") for i in range(2))
        assert p0.dtype == np.float32 and p0.shape == tuple(t.shape), k
        assert np.array_equal(p0, p1), k


@pytest.mark.parametrize("V,B,k", [(3417, 64, 20), (20034, 33, 20), (40, 5, 20), (100003, 3, 10)])
def test_hip_topk_with_seen_mask_equals_torch(V, B, k):
    """bsarec_topk_seen (the reference's `rating_pred[seen] = 0` + argpartition / argsort of the 20 best, src/trainers.py:134-149,
    as one HIP launch): same item lists and scores as zeroing + torch.topk; equal scores (the zeros) go to the smaller id."""
    from bsarec_amd import _lib as Lb
    lib = Lb.load()
    g = torch.Generator(device="cuda").manual_seed(V)
    scores = torch.randn(B, V, device="cuda", generator=g)
    rng = np.random.default_rng(V)
    rows = [np.unique(rng.integers(0, V, size=int(rng.integers(0, min(V, 400))))) for _ in range(B + 3)]
    indptr = torch.as_tensor(np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64), device="cuda")
    indices = torch.as_tensor(np.concatenate(rows).astype(np.int64), device="cuda")
    users = torch.as_tensor(rng.permutation(B + 3)[:B].astype(np.int64), device="cuda")
    want = scores.clone()
    for b in range(B):
        u = int(users[b])
        want[b, indices[int(indptr[u]):int(indptr[u + 1])]] = 0.0
    got_idx = torch.empty(B, k, dtype=torch.int64, device="cuda")
    got_val = torch.empty(B, k, dtype=torch.float32, device="cuda")
    work = scores.clone()
    Lb.check(lib.bsarec_topk_seen(work.data_ptr(), work.stride(0), B, V, users.data_ptr(), indptr.data_ptr(), indices.data_ptr(), k,
                                  got_idx.data_ptr(), got_val.data_ptr(), torch.cuda.current_stream().cuda_stream), "bsarec_topk_seen")
    torch.cuda.synchronize()
    assert torch.equal(work, want)                                   # the masked scores are what the reference would hold
    # reference order: value descending, ties (the zeros) by item id ascending
    key = torch.argsort(torch.arange(V, device="cuda").expand(B, V), dim=1, stable=True)
    order = torch.sort(want, dim=1, descending=True, stable=True).indices     # stable: equal scores keep ascending id order
    assert torch.equal(got_idx, order[:, :k])
    assert torch.equal(got_val, torch.gather(want, 1, order[:, :k]))
    tv = torch.topk(want, k, dim=1).values
    assert torch.equal(got_val, tv)
