"""BERT4Rec on the GPU: the bidirectional encoder (plan option bidirectional, all three mask sites) against the oracle under the
padding-only mask, the whole cloze step (mask -> encoder -> head -> backward) against the fp64/numpy chain of cloze_ref, the
prediction path, the rankings and a short run through the driver."""
import argparse
import ast
import logging

import numpy as np
import pytest

from conftest import rel_l2
import cloze_ref as R

pytestmark = pytest.mark.gpu
V = 131


def _args(d=64, L=50, heads=2, B=9, ph=0.4, pa=0.3, **kw):
    return argparse.Namespace(item_size=V, hidden_size=d, max_seq_length=L, batch_size=B, hidden_dropout_prob=ph,
                              attention_probs_dropout_prob=pa, num_hidden_layers=2, num_attention_heads=heads, hidden_act="gelu",
                              initializer_range=0.02, c=3, seed=42, **kw)


def _oracle_cfg(a):
    from oracle import bsarec_oracle as O
    return O.Config(item_size=V + 1, hidden_size=a.hidden_size, max_seq_length=a.max_seq_length, num_hidden_layers=2,
                    num_attention_heads=a.num_attention_heads, c=3, alpha=0.0, hidden_dropout_prob=a.hidden_dropout_prob,
                    attention_probs_dropout_prob=a.attention_probs_dropout_prob)


def _model(a, seed=3):
    """A BERT4RecModel on the GPU holding the oracle's init_params (table [V + 1, d]), and those parameters."""
    import torch
    from oracle import bsarec_oracle as O
    from bsarec_amd import BERT4RecModel, BSARecModel
    params = O.init_params(_oracle_cfg(a), seed=seed)
    m = BERT4RecModel(a)
    BSARecModel.load_state_dict(m, {k: torch.from_numpy(v) for k, v in params.items()})
    return m.cuda(), params


def _ids(B, L, rng, hi=V):
    """Row 0 empty, row 1 full, the rest of random length, left-padded."""
    ids = np.zeros((B, L), dtype=np.int64)
    for b in range(B):
        n = 0 if b == 0 else (L if b == 1 else int(rng.integers(1, L + 1)))
        if n:
            ids[b, L - n:] = rng.integers(1, hi, size=n)
    return ids


def _check_grads(m, G, gate=2e-4):
    for name, p in m.named_parameters():
        if name.endswith("key.bias"):
            continue
        if ".filter_layer." in name:                              # alpha = 0: the frequency branch gets exactly nothing
            assert p.grad is None or float(p.grad.abs().max()) == 0.0, name
            assert not np.any(G[name]), name
            continue
        e = rel_l2(p.grad.cpu().numpy(), G[name])
        assert e <= gate, (name, e)


ENCODER_CASES = [(64, 50, 2, dict()), (64, 50, 2, dict(no_fused=1)), (64, 20, 1, dict()), (64, 64, 4, dict()),
                 (32, 12, 4, dict(no_fused=1)), (64, 50, 2, dict(chain_kernels=1))]


@pytest.mark.parametrize("d,L,heads,opts", ENCODER_CASES, ids=lambda v: "-".join(f"{k}" for k in v) if isinstance(v, dict) else str(v))
def test_bidirectional_encoder_vs_patched_oracle(d, L, heads, opts):
    """d/d(params) of sum(out * W) for a random W over ALL positions, dropout on, ids holding the mask token: outputs 2e-4 absolute
    on real rows, every gradient 2e-4 relative L2 (key.bias skipped: its gradient is zero up to rounding)."""
    import torch
    from oracle import bsarec_oracle as O
    from bsarec_amd import _lib as Lb
    old = Lb.set_default_options(**opts) if opts else {}
    try:
        B = 9
        a = _args(d, L, heads, B)
        m, params = _model(a)
        assert Lb.load().bsarec_plan_is_fused(m._plan(B).handle) == (0 if opts.get("no_fused") else 1)
        rng = np.random.default_rng(3)
        ids = _ids(B, L, rng)
        ids[1, ::4] = V                                           # the mask token as an input id
        W = rng.normal(0, 1, (B, L, d)).astype(np.float32)
        m.train()
        m.set_seed(77)
        out = m(torch.from_numpy(ids).cuda())
        step = int(m._state[1].item())
        (out * torch.from_numpy(W).cuda()).sum().backward()
        d_outs = [np.zeros_like(W) for _ in range(2)] + [W]
        with R.bidirectional_oracle():
            _, _, G, outs = O.loss_and_grads(params, _oracle_cfg(a), ids, None, O.DropoutSpec(True, 77, step), d_outs=d_outs,
                                             head=R.null_head)
            causal_free = outs[-1]
        causal = O.forward(params, _oracle_cfg(a), ids, O.DropoutSpec(True, 77, step))[0][-1]
        real = ids > 0
        got = out.detach().cpu().numpy()
        assert np.abs(causal - causal_free)[real].max() > 1e-2    # the two masks differ on these inputs
        err = np.abs(got - causal_free)[real].max()
        print(f"bert4rec encoder d={d} L={L} heads={heads} {opts}: out {err:.2e}")
        assert err <= 2e-4
        _check_grads(m, G)
        assert len(m._slots_busy) == 0
    finally:
        if old:
            Lb.set_default_options(**old)


def test_causal_plans_keep_their_outputs_when_a_bidirectional_plan_exists():
    """The option belongs to a plan: a SASRec model beside a BERT4Rec model still runs the causal mask."""
    import torch
    from oracle import bsarec_oracle as O
    from bsarec_amd import SASRecModel, BSARecModel
    a = _args(ph=0.0, pa=0.0)
    m, params = _model(a)
    sa = _args(ph=0.0, pa=0.0)
    sa.item_size = V + 1
    s = SASRecModel(sa)
    BSARecModel.load_state_dict(s, {k: torch.from_numpy(v) for k, v in params.items()})
    s = s.cuda()
    ids = _ids(9, 50, np.random.default_rng(1))
    t = torch.from_numpy(ids).cuda()
    m.eval(), s.eval()
    bi, ca = m(t).cpu().numpy(), s(t).cpu().numpy()
    want = O.forward(params, _oracle_cfg(a), ids)[0][-1]
    real = ids > 0
    assert np.abs(ca - want)[real].max() <= 2e-4
    assert np.abs(bi - want)[real].max() > 1e-2


@pytest.mark.parametrize("ph,pa", [(0.0, 0.0), (0.4, 0.3)], ids=["nodrop", "drop"])
def test_cloze_step_vs_reference_chain(ph, pa):
    """calculate_loss().backward() against: the reference mask -> the oracle under the padding-only mask -> the reference head
    -> loss_and_grads(d_outs=...).  Loss 5e-6 relative, every gradient 2e-4 relative L2, the table's [V + 1, d] gradient with
    its mask-token row."""
    import torch
    from oracle import bsarec_oracle as O
    B, L, d = 9, 50, 64
    a = _args(d, L, 2, B, ph, pa, mask_ratio=0.2)
    m, params = _model(a)
    assert m.mask_slots == 20 and m.mask_token == V and m.item_embeddings.weight.shape == (V + 1, d)
    rng = np.random.default_rng(11)
    ids = _ids(B, L, rng)
    ans = rng.integers(1, V, size=B).astype(np.int64)
    m.train()
    m.set_seed(77)
    before = int(m._state[1].item())
    loss = m.calculate_loss(torch.from_numpy(ids).cuda(), torch.from_numpy(ans).cuda())
    step = int(m._state[1].item())
    assert step == before + 1                                     # advanced once
    m.zero_grad()
    loss.backward()
    seq = np.concatenate([ids[:, 1:], ans[:, None]], axis=1)
    masked, rows, targets, n = R.cloze_mask(seq, 0.2, 20, 77, step, V)
    assert 0 < n < B * 20 and (masked == V).sum() >= n
    cfg, drop = _oracle_cfg(a), O.DropoutSpec(True, 77, step)
    with R.bidirectional_oracle():
        outs, _ = O.forward(params, cfg, masked, drop)
        rloss, _, dh, dE = R.cloze_head(outs[-1].reshape(B * L, d), params["item_embeddings.weight"][:V], rows, targets, n)
        d_outs = [np.zeros((B, L, d), np.float32) for _ in range(2)] + [dh.reshape(B, L, d).astype(np.float32)]
        _, _, G, _ = O.loss_and_grads(params, cfg, masked, None, drop, d_outs=d_outs, head=R.null_head)
    G["item_embeddings.weight"][:V] += dE.astype(np.float32)
    e = abs(loss.item() - rloss) / abs(rloss)
    print(f"bert4rec step drop=({ph},{pa}): loss {loss.item():.6f} ref {rloss:.6f} rel {e:.2e} n {n}")
    assert e <= 5e-6
    assert np.abs(G["item_embeddings.weight"][V]).max() > 0      # the mask-token row has a (lookup) gradient
    _check_grads(m, G)
    assert len(m._slots_busy) == 0
    # eval mode: the current step's masking, no dropout, nothing advanced
    m.eval()
    with torch.no_grad():
        l1 = m.calculate_loss(torch.from_numpy(ids).cuda(), torch.from_numpy(ans).cuda())
        l2 = m.calculate_loss(torch.from_numpy(ids).cuda(), torch.from_numpy(ans).cuda())
    assert int(m._state[1].item()) == step and torch.equal(l1, l2)
    with R.bidirectional_oracle():
        outs, _ = O.forward(params, cfg, masked, O.DropoutSpec(False))
    eloss = R.cloze_head(outs[-1].reshape(B * L, d), params["item_embeddings.weight"][:V], rows, targets, n)[0]
    assert abs(l1.item() - eloss) <= 5e-6 * abs(eloss)


def test_last_hidden_is_the_mask_position_and_rankings_hold_no_mask_token():
    import scipy.sparse as sp
    import torch
    from bsarec_amd import data as Dm, main as M
    from bsarec_amd.trainer import Trainer
    a = _args(ph=0.0, pa=0.0)
    m, _ = _model(a)
    m.eval()
    ids = _ids(9, 50, np.random.default_rng(2))
    t = torch.from_numpy(ids).cuda()
    shifted = torch.cat((t[:, 1:], torch.full((9, 1), V, dtype=torch.int64, device="cuda")), dim=1)
    want = m(shifted)[:, -1].cpu().numpy()
    got = m.last_hidden(t).cpu().numpy()
    assert rel_l2(got, want) <= 2e-5
    assert np.array_equal(m.predict(t).cpu().numpy(), got)
    assert m.catalogue_weight().shape == (V, 64) and not m.catalogue_weight().requires_grad
    with pytest.raises(RuntimeError, match="BERT4Rec steps through"):
        m.train_step(t, t[:, 0])
    # rankings: the table without the mask-token row
    Lq = 50
    seqs = Dm.synth_ml1m_like(seed=5, n_users=60, n_items=V - 1)
    args = M.parse_args(["--model_type", "BERT4Rec", "--max_seq_length", str(Lq), "--batch_size", "64"])
    args.item_size = V
    dev = torch.device("cuda", torch.cuda.current_device())
    dls = [Dm.DeviceBatches(*Dm.eval_table(seqs, Lq, s), 64, dev, shuffle=False) for s in ("valid", "valid", "test")]
    for split in ("valid", "test"):
        indptr, cols = Dm.seen_csr(seqs, split)
        setattr(args, f"{split}_rating_matrix", sp.csr_matrix((np.ones(len(cols)), cols, indptr), shape=(len(seqs), V)))
    args.train_matrix = args.valid_rating_matrix
    with torch.no_grad():
        m.item_embeddings.weight[V] = 50.0                       # a mask-token row that would win every ranking
    tr = Trainer(m, dls[0], dls[1], dls[2], args)
    users, inputs, answers = (torch.as_tensor(x).to(dev) for x in Dm.eval_table(seqs, Lq, "valid"))
    pred = tr.topk_full(users[:32], inputs[:32], k=20)
    assert pred.shape == (32, 20) and int(pred.max()) < V and int(pred.min()) >= 0
    ranks = tr.answer_ranks(users[:32], inputs[:32], answers[:32])
    assert int(ranks.min()) >= 0 and int(ranks.max()) < V
    scores, _ = tr.valid(0)                                      # full_logits is None: the default path takes topk_full
    assert len(scores) == 6 and np.isfinite(scores).all()
    with pytest.raises(ValueError, match="BERT4Rec: single GPU only"):
        Trainer(m, None, None, None, args, process_group=object())


def test_bert4rec_trains_through_the_driver():
    """Three epochs of --model_type BERT4Rec on 600 synthetic users: the loss falls, the metrics are finite and above chance.
    A sanity band, not a known answer."""
    from bsarec_amd import data as Dm, main as M
    msgs = []

    class Grab(logging.Handler):
        def emit(self, rec):
            msgs.append(rec.msg)
    logger = logging.getLogger("bert4rec_main")
    logger.setLevel(logging.INFO)
    logger.propagate = False
    logger.addHandler(Grab())
    seqs = Dm.synth_ml1m_like(seed=5, n_users=600, n_items=300)
    args = M.parse_args(["--model_type", "BERT4Rec", "--mask_ratio", "0.2", "--max_seq_length", "50", "--batch_size", "256",
                         "--epochs", "3", "--patience", "100", "--hidden_dropout_prob", "0.2",
                         "--attention_probs_dropout_prob", "0.2"])
    scores, info, epochs, secs = M.run(args, seqs, logger)
    losses = [float(ast.literal_eval(s)["rec_loss"]) for s in msgs if isinstance(s, str) and "'rec_loss'" in s]
    n_items = max(max(s) for s in seqs) + 1
    print(f"bert4rec driver: losses {losses} scores {scores} ({secs:.1f} s)")
    assert epochs == 3 and len(losses) == 3 and np.isfinite(losses).all()
    assert losses[-1] < losses[0]
    assert len(scores) == 6 and np.isfinite(scores).all() and all(0.0 <= s <= 1.0 for s in scores)
    assert scores[2] > 10.0 / n_items                            # HR@10 above a uniform guess
