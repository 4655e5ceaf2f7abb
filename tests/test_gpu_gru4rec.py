"""GRU4RecModel on the GPU against a CPU twin in double (nn.Embedding + nn.GRU(bias=False) + nn.Linear, dropout 0): forward, BPR
loss, every parameter gradient, three Adam steps; last_hidden, the seeded dropout draws, main.run end to end, the evaluation
paths, the checkpoint round trip and the trainer's refusals.  V = 301, d = 64, N = 2, L = 20, B = 33."""
import argparse
import functools
import logging

import numpy as np
import pytest

from conftest import rel_l2

pytestmark = pytest.mark.gpu
OUT_GATE, GRAD_GATE = 2e-5, 2e-4
V, D, N, L, B = 301, 64, 2, 20, 33


def _args(H, **kw):
    a = argparse.Namespace(item_size=V, hidden_size=D, gru_hidden_size=H, num_hidden_layers=N, max_seq_length=L,
                           hidden_dropout_prob=0.0, initializer_range=0.02, lr=1e-3, adam_beta1=0.9, adam_beta2=0.999,
                           weight_decay=0.0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _twin(H):
    import torch

    class Twin(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.item_embeddings = torch.nn.Embedding(V, D)
            self.gru_layers = torch.nn.GRU(D, H, N, bias=False, batch_first=True)
            self.dense = torch.nn.Linear(H, D)

        def forward(self, ids):
            return self.dense(self.gru_layers(self.item_embeddings(ids))[0])

        def calculate_loss(self, ids, pos, neg):
            s = self.forward(ids)[:, -1]
            E = self.item_embeddings
            return -torch.log(torch.sigmoid((s * E(pos)).sum(-1) - (s * E(neg)).sum(-1)) + 1e-10).mean()
    return Twin().double()


def _batch():
    import torch
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(1, V, (B, L), generator=g)
    ids[:5, :7] = 0                                           # padding in front, not masked by this model
    pos = torch.randint(1, V, (B,), generator=g)
    neg = torch.randint(1, V, (B,), generator=g)
    pos[0], neg[1] = ids[0, -1], ids[1, -1]                   # rows of the table that the lookup and the head both touch
    return ids, pos, neg


@functools.lru_cache(maxsize=None)
def _pair(H):
    """The model (GPU, trained-size weights: a few times the init so that the gates leave the linear range), its twin with the
    same parameters, and the twin's forward, loss and gradients, computed once."""
    import torch
    from bsarec_amd import GRU4RecModel
    torch.manual_seed(7 + H)
    m = GRU4RecModel(_args(H))
    with torch.no_grad():
        m.item_embeddings.weight.mul_(25.0)
        m.dense.weight.mul_(10.0)
        m.dense.bias.normal_(0.0, 0.1)
    twin = _twin(H)
    twin.load_state_dict(m.state_dict())
    m = m.cuda()
    ids, pos, neg = _batch()
    out = twin(ids).detach().numpy()
    loss = twin.calculate_loss(ids, pos, neg)
    loss.backward()
    grads = {k: p.grad.numpy().copy() for k, p in twin.named_parameters()}
    return m, twin, out, loss.item(), grads


@pytest.mark.parametrize("H", [64, 96])
def test_forward_loss_and_gradients_against_the_twin(H):
    import torch
    m, twin, rout, rloss, rgrads = _pair(H)
    ids, pos, neg = (t.cuda() for t in _batch())
    m.eval()
    with torch.no_grad():
        out = m(ids)
        assert torch.equal(m.predict(ids, all_sequence_output=True), out)
        assert torch.equal(m.last_hidden(ids), out[:, -1])                 # bit for bit
    e_out = rel_l2(out.cpu().numpy(), rout)
    m.train()
    m.zero_grad()
    loss = m.calculate_loss(ids, pos, neg)
    loss.backward()
    e_loss = abs(loss.item() - rloss) / abs(rloss)
    errs = {k: rel_l2(p.grad.cpu().numpy(), rgrads[k]) for k, p in m.named_parameters()}
    touched = torch.unique(torch.cat([ids.reshape(-1), pos, neg])).cpu().numpy()
    g = m.item_embeddings.weight.grad.cpu().numpy()
    both = np.array([ids[0, -1].item(), ids[1, -1].item()])
    e_both = rel_l2(g[both], rgrads["item_embeddings.weight"][both])
    print(f"gru4rec H={H}: out {e_out:.2e} loss {loss.item():.7f} rel {e_loss:.2e} rows(lookup+head) {e_both:.2e} " +
          " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    assert list(errs) == [k for k, _ in twin.named_parameters()]
    assert e_out <= OUT_GATE
    assert e_loss <= 5e-6
    for k, v in errs.items():
        assert v <= GRAD_GATE, (k, v)
    assert e_both <= GRAD_GATE
    rest = np.setdiff1d(np.arange(V), touched)
    assert not g[rest].any()
    # the differentiable full forward: d(out) / d(parameters) against the twin for a linear functional of the output
    m.zero_grad()
    twin.zero_grad()
    c = torch.Generator().manual_seed(2)
    coef = torch.randn(B, L, D, generator=c, dtype=torch.float64)
    (twin(ids.cpu()) * coef).sum().backward()
    (m(ids) * coef.float().cuda()).sum().backward()
    for k, p in m.named_parameters():
        assert rel_l2(p.grad.cpu().numpy(), dict(twin.named_parameters())[k].grad.numpy()) <= GRAD_GATE, k
    twin.zero_grad()


@pytest.mark.parametrize("H", [64, 96])
def test_three_adam_steps_against_the_twin(H):
    import copy
    import torch
    m0, twin0 = _pair(H)[:2]
    m, twin = copy.deepcopy(m0), copy.deepcopy(twin0)
    m.gru_layers.reflatten()
    m.train()
    ids, pos, neg = _batch()
    om = torch.optim.Adam(m.parameters(), lr=1e-3)
    ot = torch.optim.Adam(twin.parameters(), lr=1e-3)
    for _ in range(3):
        om.zero_grad()
        m.calculate_loss(ids.cuda(), pos.cuda(), neg.cuda()).backward()
        om.step()
        ot.zero_grad()
        twin.calculate_loss(ids, pos, neg).backward()
        ot.step()
    flat = m.gru_layers._flat
    off = 0
    for (k, p), (_, q) in zip(m.named_parameters(), twin.named_parameters()):
        e = rel_l2(p.detach().cpu().numpy(), q.detach().numpy())
        print(f"adam x3 H={H} {k}: {e:.2e}")
        assert e <= 2e-4, (k, e)
        assert not torch.equal(p.detach().cpu(), dict(m0.named_parameters())[k].detach().cpu())       # it moved
        if k != "item_embeddings.weight":                     # updated in place: still views of the flat array
            assert p.data_ptr() == flat.data_ptr() + 4 * off, k
            off += p.numel()


def test_dropout_draws_follow_the_seed():
    import torch
    from bsarec_amd import GRU4RecModel
    torch.manual_seed(1)
    m = GRU4RecModel(_args(64, hidden_dropout_prob=0.5)).cuda()
    ids = _batch()[0].cuda()
    m.train()
    with torch.no_grad():
        m.set_seed(5)
        a = m(ids)
        m.set_seed(5)
        b = m(ids)
        c = m(ids)                                            # the next draw of the same stream
        m.set_seed(6)
        d = m(ids)
        m.eval()
        e1, e2 = m(ids), m(ids)
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, d)
    assert torch.equal(e1, e2) and not torch.equal(e1, a)
    with pytest.raises(RuntimeError, match="MI355X"):
        m(ids.cpu())


def _setup(argv):
    """What main.run builds before its epoch loop, for a GRU4Rec run on 200 users and 300 items."""
    import scipy.sparse as sp
    import torch
    from bsarec_amd import data as Dm, main as M
    from bsarec_amd.trainer import Trainer
    seqs = Dm.synth_ml1m_like(seed=5, n_users=200, n_items=300)
    args = M.parse_args(["--model_type", "GRU4Rec", "--max_seq_length", str(L), "--batch_size", "256", "--epochs", "2",
                         "--patience", "100"] + argv)
    args.item_size = max(max(s) for s in seqs) + 1
    dev = torch.device("cuda", torch.cuda.current_device())
    u, x, a = Dm.train_table(seqs, L)
    train_dl = Dm.DeviceBatches(u, x, a, args.batch_size, dev, shuffle=True, seed=args.seed)
    eval_dl = Dm.DeviceBatches(*Dm.eval_table(seqs, L, "valid"), args.batch_size, dev, shuffle=False)
    test_dl = Dm.DeviceBatches(*Dm.eval_table(seqs, L, "test"), args.batch_size, dev, shuffle=False)
    for split in ("valid", "test"):
        indptr, cols = Dm.seen_csr(seqs, split)
        setattr(args, f"{split}_rating_matrix", sp.csr_matrix((np.ones(len(cols)), cols, indptr), shape=(len(seqs), args.item_size)))
    torch.manual_seed(args.seed)
    model = M.MODEL_DICT[args.model_type.lower()](args=args)
    train_dl.enable_negatives(seqs, args.item_size)
    model.set_seed(args.seed)
    return seqs, args, model, Trainer(model, train_dl, eval_dl, test_dl, args)


def test_main_run_end_to_end():
    import ast
    from bsarec_amd import data as Dm, main as M
    msgs = []

    class Grab(logging.Handler):
        def emit(self, rec):
            msgs.append(rec.msg)
    logger = logging.getLogger("gru4rec_main")
    logger.setLevel(logging.INFO)
    logger.propagate = False
    logger.addHandler(Grab())
    seqs = Dm.synth_ml1m_like(seed=5, n_users=200, n_items=300)
    args = M.parse_args(["--model_type", "GRU4Rec", "--gru_hidden_size", "64", "--max_seq_length", str(L), "--batch_size", "256",
                         "--epochs", "2", "--patience", "100"])
    scores, info, epochs, secs = M.run(args, seqs, logger)
    losses = [float(ast.literal_eval(m)["rec_loss"]) for m in msgs if isinstance(m, str) and "'rec_loss'" in m]
    assert epochs == 2 and len(losses) == 2 and np.isfinite(losses).all()
    assert len(scores) == 6 and np.isfinite(scores).all() and all(0.0 <= s <= 1.0 for s in scores)


def test_evaluation_paths_agree_and_checkpoint_round_trip(tmp_path):
    import torch
    seqs, args, model, tr = _setup([])
    tr.train(0)
    dense, _ = tr.test(0)                                     # no full_logits: the default path takes topk_full
    args.eval_full_rank = "fused"
    fused, _ = tr.test(0)
    args.eval_full_rank = "rank"
    rank, _ = tr.test(0)
    assert len(fused) == 6 and np.isfinite(fused).all()
    assert list(dense) == list(fused)
    assert np.allclose(rank[:6], fused, rtol=0, atol=1e-12) and len(rank) == 7          # + MRR
    args.eval_negatives = 50
    sampled, _ = tr.valid(0)
    assert len(sampled) == 6 and np.isfinite(sampled).all()
    del args.eval_negatives
    # save -> load, bit for bit, into the arrays the kernels read
    path = str(tmp_path / "gru4rec.pt")
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    tr.save(path)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(1.0)
    tr.load(path)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
    args.eval_full_rank = "fused"
    assert list(tr.test(0)[0]) == list(fused)


def test_trainer_refusals():
    from bsarec_amd import GRU4RecModel
    from bsarec_amd.trainer import Trainer
    m = GRU4RecModel(_args(64))
    with pytest.raises(ValueError, match="GRU4Rec: single GPU only"):
        Trainer(m, None, None, None, _args(64), process_group=object())
    with pytest.raises(ValueError, match="GRU4Rec"):
        Trainer(m, None, None, None, _args(64, train_negatives=8))
