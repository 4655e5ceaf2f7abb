"""FEARecModel on the GPU against its fp64 twin (fearec_ref.Twin, the same state_dict, dropout 0): the loss and every parameter's
gradient over the ssl variants, the regulariser, the spatial branch and the torch / HIP heads; last_hidden; dropout; a short
Trainer run.  V = 50, d = 16, L = 12, N = 2, heads = 2, B = 4.

Gates: those of test_duorec.py's GPU comparison -- the loss to 5e-6 relative, every gradient to 1e-4 rel-L2; a gradient that is
zero in the twin to fp64 rounding (<= 1e-12: the query / key biases of a layer whose band leaves out DC, at spatial_ratio 0) must
be <= 1e-6 in the model, as test_duorec.py asks of key.bias.  The twin asserts the margin condition (1e-4 of max|m|) on its own
choice of delays, in every attention call."""
import argparse

import numpy as np
import pytest

import fearec_ref as R

pytestmark = pytest.mark.gpu
LOSS_GATE, GRAD_GATE, ZERO_REF, ZERO_GOT = 5e-6, 1e-4, 1e-12, 1e-6
V, D, L, B = 50, 16, 12, 4


def _args(**kw):
    base = dict(item_size=V, hidden_size=D, max_seq_length=L, batch_size=B, hidden_dropout_prob=0.0,
                attention_probs_dropout_prob=0.0, num_hidden_layers=2, num_attention_heads=2, hidden_act="gelu",
                initializer_range=0.1, seed=1, lr=1e-3, adam_beta1=0.9, adam_beta2=0.999, weight_decay=0.0)
    base.update(kw)
    return argparse.Namespace(**base)


def _batch(seed=0):
    """ids, same_target ids (left-padded, lengths 3 .. L), answers."""
    rng = np.random.default_rng(seed)
    ids, sem = np.zeros((B, L), dtype=np.int64), np.zeros((B, L), dtype=np.int64)
    for a, lens in ((ids, (L, 3, 7, 10)), (sem, (5, L, 9, 4))):
        for b, n in enumerate(lens):
            a[b, L - n:] = rng.integers(1, V, size=n)
    return ids, sem, rng.integers(1, V, size=B)


def _model(args, seed=3):
    import torch
    from bsarec_amd import FEARecModel
    torch.manual_seed(seed)
    m = FEARecModel(args)
    with torch.no_grad():                                              # LayerNorms and biases off their init, so that they matter
        for k, p in m.named_parameters():
            if "LayerNorm" in k or k.endswith(".bias"):
                p.add_(0.1 * torch.randn_like(p))
    return m


CASES = [("us_x", True, "us_x", 0.1, "torch", "torch"), ("us_x", True, "us_x", 0.0, "hip", "hip"),
         ("us_x", False, "us_x", 0.1, "hip", "torch"), ("us_x", True, "un", 0.0, "torch", "torch"),
         ("us_x", True, "su", 0.1, "torch", "hip"), ("un", True, "us_x", 0.1, "torch", "hip"),
         ("un", True, "us_x", 0.0, "hip", "hip"), ("su", True, "us_x", 0.0, "torch", "torch"),
         ("su", False, "us_x", 0.1, "hip", "hip")]


@pytest.mark.parametrize("ssl,fredom,ftype,r,head,ce_head", CASES, ids=["-".join(map(str, c)) for c in CASES])
def test_loss_and_gradients_vs_the_fp64_twin(ssl, fredom, ftype, r, head, ce_head):
    import torch
    args = _args(ssl=ssl, fredom=fredom, fredom_type=ftype, spatial_ratio=r, duorec_head=head, duorec_ce_head=ce_head)
    m = _model(args)
    twin = R.Twin(m.state_dict(), args)
    ids, sem, ans = _batch()
    want = twin.loss(torch.from_numpy(ids), torch.from_numpy(ans), torch.from_numpy(sem))
    want.backward()
    m = m.cuda()
    m.train()
    loss = m.calculate_loss(torch.from_numpy(ids).cuda(), torch.from_numpy(ans).cuda(), None, torch.from_numpy(sem).cuda())
    m.zero_grad()
    loss.backward()
    e_loss = abs(loss.item() - want.item()) / abs(want.item())
    errs = {}
    for k, p in m.named_parameters():
        ref = twin.p[k].grad.numpy()
        got = p.grad.cpu().numpy()
        if np.abs(ref).max() <= ZERO_REF:
            errs[k] = ("abs", float(np.abs(got).max()))
        else:
            errs[k] = ("rel", R.rel_l2(got, ref))
    worst = max((e for kind, e in errs.values() if kind == "rel"), default=0.0)
    print(f"fearec {ssl} fredom={fredom}/{ftype} r={r} {head}/{ce_head}: loss {loss.item():.6f} err {e_loss:.2e}, worst gradient "
          f"{worst:.2e}, zero in the twin: {[k for k, (kind, e) in errs.items() if kind == 'abs']}")
    assert e_loss <= LOSS_GATE
    assert len(errs) == 36
    for k, (kind, e) in errs.items():
        assert e <= (GRAD_GATE if kind == "rel" else ZERO_GOT), (k, kind, e)


@pytest.mark.parametrize("r", [0.0, 0.1])
def test_last_hidden_is_the_evaluation_mode_twin(r):
    import torch
    args = _args(spatial_ratio=r)
    m = _model(args)
    twin = R.Twin(m.state_dict(), args)
    ids, _, _ = _batch(1)                    # (batch 0 has a row whose evaluation-mode choice the twin calls ambiguous)
    with torch.no_grad():
        want = twin.encode(torch.from_numpy(ids), False)[:, -1].numpy()
    m = m.cuda()
    m.train()                                                          # last_hidden is evaluation mode whatever the module's mode
    t = torch.from_numpy(ids).cuda()
    got = m.last_hidden(t)
    assert got.shape == (B, D) and not got.requires_grad
    assert R.rel_l2(got.cpu().numpy(), want) <= 2e-5
    m.eval()
    assert torch.equal(m.last_hidden(t), got) and torch.equal(m.predict(t)[:, -1], got)
    with pytest.raises(ValueError, match="max_seq_length"):
        m.last_hidden(t[:, 1:])


def test_dropout_draws_follow_the_seed():
    import torch
    args = _args(hidden_dropout_prob=0.5, attention_probs_dropout_prob=0.5)
    m = _model(args).cuda()
    m.train()
    ids, sem, ans = (torch.from_numpy(a).cuda() for a in _batch())
    losses = []
    for seed in (1, 2, 1):
        m.set_seed(seed)
        loss = m.calculate_loss(ids, ans, None, sem)
        m.zero_grad()
        loss.backward()
        assert torch.isfinite(loss) and all(torch.isfinite(p.grad).all() for p in m.parameters())
        losses.append(loss.item())
    assert losses[0] != losses[1] and losses[0] == losses[2]


def test_trainer_steps_and_evaluates():
    """Three steps and one evaluation through Trainer on toy data: the six metrics, all finite."""
    import scipy.sparse as sp
    import torch
    from bsarec_amd import data as Dm, main as M
    from bsarec_amd.trainer import Trainer
    seqs = Dm.synth_ml1m_like(seed=5, n_users=60, n_items=V - 1)
    args = M.parse_args(["--model_type", "FEARec", "--max_seq_length", str(L), "--hidden_size", str(D), "--batch_size", "32",
                         "--duorec_head", "hip", "--duorec_ce_head", "hip"])
    args.item_size = max(max(s) for s in seqs) + 1
    dev = torch.device("cuda", torch.cuda.current_device())
    u, x, a = Dm.train_table(seqs, L)
    train_dl = Dm.DeviceBatches(u[:96], x[:96], a[:96], 32, dev, shuffle=True, seed=1)
    train_dl.enable_same_target()
    dls = [Dm.DeviceBatches(*Dm.eval_table(seqs, L, s), 32, dev, shuffle=False) for s in ("valid", "test")]
    for split in ("valid", "test"):
        indptr, cols = Dm.seen_csr(seqs, split)
        setattr(args, f"{split}_rating_matrix", sp.csr_matrix((np.ones(len(cols)), cols, indptr), shape=(len(seqs), args.item_size)))
    args.train_matrix = args.valid_rating_matrix
    model = M.model_class(args.model_type)(args=args)
    model.set_seed(args.seed)
    tr = Trainer(model, train_dl, dls[0], dls[1], args)
    assert len(train_dl) == 3
    before = {k: v.clone() for k, v in tr.model.state_dict().items()}
    post = tr.train(0)
    assert np.isfinite(float(post["rec_loss"]))
    assert any(not torch.equal(v, before[k]) for k, v in tr.model.state_dict().items())
    scores, _ = tr.valid(0)
    assert len(scores) == 6 and np.isfinite(scores).all() and all(0.0 <= s <= 1.0 for s in scores)
    with pytest.raises(ValueError, match="FEARec: single GPU only"):
        Trainer(model, None, None, None, args, process_group=object())
