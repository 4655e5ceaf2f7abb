"""The fused Mamba4Rec step on the GPU (mamba_step = "fused": bsarec_mamba4rec_loss_grad / bsarec_mamba4rec_train_step) against
the step in numpy double (mamba4rec_step_ref): loss and every gradient at p = 0 and at p = 0.5 under the masks of the device state
on four shapes, the eval-mode loss against calculate_loss, three Adam steps, bit determinism with a poisoned workspace, graph
replay against eager calls, and the trainer end to end.

  shape 1  V = 301, d = 64, N = 2, L = 20, B = 33; E = 2, d_state = 16, K = 4, R = 4    two state checkpoints (every 8th step),
                                                                                     660 tokens, the layer's defaults at d = 64
  shape 2  V = 5, d = 4, N = 1, L = 1, B = 17; E = 1, d_state = 4, K = 2, R = 4         L = 1, no checkpoint, the smallest d; V < B:
                                                                                     ids and answers collide; dA_log exactly 0
  shape 3  V = 40, d = 256, N = 1, L = 3, B = 65; E = 2, d_state = 32, K = 4, R = 16    d_inner = 512, d_state = 32, L < K, B one past
                                                                                     a 64-row tile
  shape 4  V = 23, d = 100, N = 2, L = 17, B = 5; E = 2, d_state = 16, K = 3, R = 8     d no power of two, L one past a checkpoint
                                                                                     edge, K = 3

Gates: those of test_gpu_lrurec_step.py and test_gpu_mamba4rec.py -- the loss to 5e-6 relative, every gradient tensor <= 2e-4
rel-L2, the parameters after three Adam steps <= 2e-4 rel-L2."""
import argparse

import numpy as np
import pytest

import mamba_ref as R
import mamba4rec_step_ref as S
import step_harness as H

pytestmark = pytest.mark.gpu
LOSS_GATE, GRAD_GATE = 5e-6, 2e-4
SHAPES = {1: (301, 64, 2, 20, 33), 2: (5, 4, 1, 1, 17), 3: (40, 256, 1, 3, 65), 4: (23, 100, 2, 17, 5)}      # V, d, N, L, B
HYPER = {1: (2, 16, 4, 4), 2: (1, 4, 2, 4), 3: (2, 32, 4, 16), 4: (2, 16, 3, 8)}          # expand, d_state, d_conv, dt_rank
SEED = 5


def _args(shape, p=0.0, **kw):
    V, d, N, L, B = SHAPES[shape]
    E, ds, K, Rk = HYPER[shape]
    a = argparse.Namespace(item_size=V, hidden_size=d, num_hidden_layers=N, max_seq_length=L, hidden_dropout_prob=p,
                           initializer_range=0.1, lr=1e-3, adam_beta1=0.9, adam_beta2=0.999, weight_decay=0.0,
                           mamba_expand=E, mamba_d_state=ds, mamba_d_conv=K, mamba_dt_rank=Rk, mamba_step="fused")
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _batch(shape):
    V, d, N, L, B = SHAPES[shape]
    return H.block_batch(R.ragged_ids, V, L, B, 10 + shape)


def _model(shape, p=0.0, **kw):
    """A fused-step model on the GPU, LayerNorms and biases (but dt_proj's) off their init so that they matter (as
    test_gpu_mamba4rec._model); the same weights for every p and option."""
    import torch
    from bsarec_amd import Mamba4RecModel
    torch.manual_seed(7 + shape)
    m = Mamba4RecModel(_args(shape, p, **kw))
    with torch.no_grad():
        for k, q in m.named_parameters():
            if "LayerNorm" in k or (k.endswith(".bias") and "dt_proj" not in k):
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
    loss, grads, _ = S.loss_and_grads(H.params64(_model(shape)), ids, ans, SHAPES[shape][2], HYPER[shape],
                                      _mults(shape, p, seed, step))
    return loss, grads


D = H.describe(stem="mamba4rec", name="Mamba4Rec", flag="mamba_step", seed=SEED, loss_gate=LOSS_GATE,
               grad_gate=GRAD_GATE, vbl=lambda shape: (SHAPES[shape][0], SHAPES[shape][4], SHAPES[shape][3]),
               slot=lambda B, L: (B, L), args=_args, model=_model, batch=_batch, reference=_reference, mults=_mults,
               main=H.MAIN, trainer=("test_gpu_mamba4rec", None),
               train_step=lambda params, st, hb, mults: S.train_step(params, st, *hb, SHAPES[1][2], HYPER[1], mults))


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("shape", [1, 2, 3, 4])
def test_loss_and_grads_against_the_reference(shape, p):
    V, d, N, L, B = SHAPES[shape]
    m, call, loss, grads, (rloss, rgrads) = H.first_call(D, shape, p)
    assert sorted(grads) == sorted(m.state_dict()) and list(m.state_dict()) == S.keys(N, HYPER[shape], d)
    assert list(grads)[1:] == S.flat_keys(N, HYPER[shape], d)
    both = np.intersect1d(*(np.unique(a) for a in H.batch(D, shape)))          # looked up AND some row's answer
    assert len(both) >= 2
    H.check_loss_and_grads(D, shape, p, loss, grads, rloss, rgrads, both)
    if L == 1:                                                  # no earlier state: dA_log is exactly 0
        assert not grads["item_encoder.blocks.0.mamba.A_log"].any()
    H.second_call_tail(D, m, shape, p, call, loss, grads)


@pytest.mark.parametrize("p,wd", [(0.0, 0.0), (0.5, 0.0), (0.5, 0.01)])
def test_three_train_steps_against_the_reference(p, wd):
    V, d, N, L, B = SHAPES[1]
    m = H.three_adam_steps(D, p, wd)
    flat = m._wflat
    named = dict(m.named_parameters())
    off = 0
    for k in S.flat_keys(N, HYPER[1], d):                       # updated in place: still views of the flat array
        assert named[k].data_ptr() == flat.data_ptr() + 4 * off, k
        off += named[k].numel()
    assert off == flat.numel()
    for k, blk in enumerate(m.item_encoder.blocks):             # ... and each layer's array still a slice of it
        la = blk.mamba
        assert la._flat.data_ptr() == named[f"item_encoder.blocks.{k}.mamba.in_proj.weight"].data_ptr()
        assert all(q.data_ptr() == la._flat.data_ptr() + 4 * o for q, (o, n, s) in zip(la.flat_parameters(), la._slices.values()))


def test_determinism_with_a_poisoned_workspace():
    H.determinism_with_a_poisoned_workspace(D)


def test_graph_replay_is_the_next_step():
    H.graph_replay_is_the_next_step(D)


def test_main_run_with_the_fused_step(monkeypatch):
    H.main_run_with_the_fused_step(D, monkeypatch)


def test_trainer_evaluation_paths_and_checkpoint_round_trip(tmp_path):
    H.trainer_evaluation_paths_and_checkpoint_round_trip(D, tmp_path)
