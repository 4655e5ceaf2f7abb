"""The fused LRURec step on the GPU (lru_step = "fused": bsarec_lrurec_loss_grad / bsarec_lrurec_train_step) against the step in
numpy double (lrurec_step_ref): loss and every gradient at p = 0 and at p = 0.5 under the masks of the device state on four shapes,
the eval-mode loss against calculate_loss, three Adam steps, bit determinism with a poisoned workspace, graph replay against eager
calls, and the trainer end to end.

  shape 1  V = 301, d = 64, N = 2, L = 20, B = 33   660 tokens: no multiple of the scatter chunk; ragged padding
  shape 2  V = 5, d = 4, N = 1, L = 1, B = 17       L = 1 and the smallest d; V < B: ids and answers repeat and collide
  shape 3  V = 40, d = 256, N = 1, L = 3, B = 65    64 float4 lanes per row, 4 d = 1024, B one past a 64-row tile
  shape 4  V = 23, d = 100, N = 2, L = 17, B = 5    d no power of two, L one past a scan chunk edge

Gates: those of test_gpu_gru4rec_step.py and test_gpu_lrurec.py -- the loss to 5e-6 relative, every gradient tensor <= 2e-4 rel-L2,
the parameters after three Adam steps <= 2e-4 rel-L2."""
import argparse

import numpy as np
import pytest

import lru_ref as R
import lrurec_step_ref as S
import step_harness as H

pytestmark = pytest.mark.gpu
LOSS_GATE, GRAD_GATE = 5e-6, 2e-4
SHAPES = {1: (301, 64, 2, 20, 33), 2: (5, 4, 1, 1, 17), 3: (40, 256, 1, 3, 65), 4: (23, 100, 2, 17, 5)}
SEED = 5


def _args(shape, p=0.0, **kw):
    V, d, N, L, B = SHAPES[shape]
    a = argparse.Namespace(item_size=V, hidden_size=d, num_hidden_layers=N, max_seq_length=L, hidden_dropout_prob=p,
                           initializer_range=0.1, lr=1e-3, adam_beta1=0.9, adam_beta2=0.999, weight_decay=0.0, lru_step="fused")
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _batch(shape):
    V, d, N, L, B = SHAPES[shape]
    return H.block_batch(R.ragged_ids, V, L, B, 10 + shape)


def _model(shape, p=0.0, **kw):
    """A fused-step model on the GPU, LayerNorms and biases off their init so that they matter (as test_gpu_lrurec._model); the
    same weights for every p and option."""
    import torch
    from bsarec_amd import LRURecModel
    torch.manual_seed(7 + shape)
    m = LRURecModel(_args(shape, p, **kw))
    with torch.no_grad():
        for k, q in m.named_parameters():
            if "LayerNorm" in k or k.endswith(".bias"):
                q.add_(0.1 * torch.randn_like(q))
    m = m.cuda()
    m.train()
    m.set_seed(SEED)
    return m


def _mults(shape, p, seed, step):
    V, d, N, L, B = SHAPES[shape]
    return S.dropout_mults(B, L, d, N, p, seed, step)


def _reference(shape, p, seed, step):
    """Loss and gradients of the reference at the model's initial weights, under the masks of (seed, step)."""
    ids, ans = H.batch(D, shape)
    loss, grads, _ = S.loss_and_grads(H.params64(_model(shape)), ids, ans, SHAPES[shape][2], _mults(shape, p, seed, step))
    return loss, grads


D = H.describe(stem="lrurec", name="LRURec", flag="lru_step", seed=SEED, loss_gate=LOSS_GATE,
               grad_gate=GRAD_GATE, vbl=lambda shape: (SHAPES[shape][0], SHAPES[shape][4], SHAPES[shape][3]),
               slot=lambda B, L: (B, L), args=_args, model=_model, batch=_batch, reference=_reference, mults=_mults,
               main=H.MAIN, trainer=("test_gpu_lrurec", None),
               train_step=lambda params, st, hb, mults: S.train_step(params, st, *hb, SHAPES[1][2], mults))


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("shape", [1, 2, 3, 4])
def test_loss_and_grads_against_the_reference(shape, p):
    V, d, N, L, B = SHAPES[shape]
    m, call, loss, grads, (rloss, rgrads) = H.first_call(D, shape, p)
    assert list(grads) == list(m.state_dict()) == S.keys(N, d)
    both = np.intersect1d(*(np.unique(a) for a in H.batch(D, shape)))          # looked up AND some row's answer
    assert len(both) >= 2
    H.check_loss_and_grads(D, shape, p, loss, grads, rloss, rgrads, both)
    H.second_call_tail(D, m, shape, p, call, loss, grads)


@pytest.mark.parametrize("p,wd", [(0.0, 0.0), (0.5, 0.0), (0.5, 0.01)])
def test_three_train_steps_against_the_reference(p, wd):
    m = H.three_adam_steps(D, p, wd)
    flat = m._wflat
    off = 0
    for k, q in m.named_parameters():
        if k != "item_embeddings.weight":                       # updated in place: still views of the flat array
            assert q.data_ptr() == flat.data_ptr() + 4 * off, k
            off += q.numel()
    assert off == flat.numel()
    for blk in m.item_encoder.blocks:                           # ... and each layer's array still a slice of it
        la = blk.lru
        assert all(q.data_ptr() == la._flat.data_ptr() + 4 * o for q, (o, n, s) in zip(la.flat_parameters(), la._slices.values()))


def test_determinism_with_a_poisoned_workspace():
    H.determinism_with_a_poisoned_workspace(D)


def test_graph_replay_is_the_next_step():
    H.graph_replay_is_the_next_step(D)


def test_main_run_with_the_fused_step(monkeypatch):
    H.main_run_with_the_fused_step(D, monkeypatch)


def test_trainer_evaluation_paths_and_checkpoint_round_trip(tmp_path):
    H.trainer_evaluation_paths_and_checkpoint_round_trip(D, tmp_path)
