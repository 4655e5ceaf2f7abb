"""The fused GRU4Rec step on the GPU (gru_step = "fused": bsarec_gru4rec_loss_grad / bsarec_gru4rec_train_step) against the step in
numpy double (gru4rec_step_ref): loss and every gradient at p = 0 and p = 0.5 on three shapes, three Adam steps, bit determinism
with a poisoned workspace, graph replay against eager calls, and the trainer end to end.

  shape 1  V = 301, d = 64, H = 64, N = 2, L = 20, B = 33   660 tokens: no multiple of the scatter chunk; B one past two 16-row tiles
  shape 2  V = 5, d = 36, H = 32, N = 1, L = 1, B = 17      d no multiple of 32, L = 1, every row of the table hit many times
  shape 3  V = 40, d = 256, H = 128, N = 1, L = 3, B = 65   the widest rows (64 float4 lanes per row)"""
import argparse

import numpy as np
import pytest

import gru4rec_step_ref as S
import step_harness as H

pytestmark = pytest.mark.gpu
LOSS_GATE, GRAD_GATE = 5e-6, 2e-4
SHAPES = {1: (301, 64, 64, 2, 20, 33), 2: (5, 36, 32, 1, 1, 17), 3: (40, 256, 128, 1, 3, 65)}
SEED = 5


def _args(shape, p=0.0, **kw):
    V, d, H, N, L, B = SHAPES[shape]
    a = argparse.Namespace(item_size=V, hidden_size=d, gru_hidden_size=H, num_hidden_layers=N, max_seq_length=L,
                           hidden_dropout_prob=p, initializer_range=0.02, lr=1e-3, adam_beta1=0.9, adam_beta2=0.999,
                           weight_decay=0.0, gru_step="fused")
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _batch(shape):
    V, d, H_, N, L, B = SHAPES[shape]
    return H.pairwise_batch(V, L, B)


def _model(shape, p=0.0, **kw):
    """A fused-step model on the GPU with trained-size weights (as test_gpu_gru4rec._pair: the gates leave the linear range); the
    same weights for every p and option."""
    import torch
    from bsarec_amd import GRU4RecModel
    torch.manual_seed(7 + shape)
    m = GRU4RecModel(_args(shape, p, **kw))
    with torch.no_grad():
        m.item_embeddings.weight.mul_(25.0)
        m.dense.weight.mul_(10.0)
        m.dense.bias.normal_(0.0, 0.1)
    m = m.cuda()
    m.train()
    m.set_seed(SEED)
    return m


_params = H.params64                                         # test_gpu_gru4rec_cand takes _batch, _model and _params from here


def _mult(shape, p, seed, step):
    V, d, H_, N, L, B = SHAPES[shape]
    return S.dropout_mult(B, L, d, p, seed, step)


def _reference(shape, p, seed, step):
    """Loss and gradients of the reference at the model's initial weights, under the mask of (seed, step)."""
    V, d, H_, N, L, B = SHAPES[shape]
    return S.loss_and_grads(H.params64(_model(shape)), *H.host(D, shape), H_, N, _mult(shape, p, seed, step))


D = H.describe(stem="gru4rec", name="GRU4Rec", flag="gru_step", seed=SEED, loss_gate=LOSS_GATE,
               grad_gate=GRAD_GATE, vbl=lambda shape: (SHAPES[shape][0], SHAPES[shape][5], SHAPES[shape][4]),
               slot=lambda B, L: (B, L), args=_args, model=_model, batch=_batch, reference=_reference, mults=_mult,
               train_step=lambda params, st, hb, mult: S.train_step(params, st, *hb, SHAPES[1][2], SHAPES[1][3], mult),
               eval_kw=dict(train=False), main=dict(H.MAIN, argv=["--gru_hidden_size", "64"] + H.MAIN["argv"]),
               trainer=("test_gpu_gru4rec", "dense.weight"))


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("shape", [1, 2, 3])
def test_loss_and_grads_against_the_reference(shape, p):
    import torch
    V, d, H_, N, L, B = SHAPES[shape]
    m, call, loss, grads, (rloss, rgrads) = H.first_call(D, shape, p)
    ids, pos, neg = call[0]
    assert list(grads) == list(m.state_dict()) == S.keys(N)
    both = np.array([ids[6, -1].item(), ids[7, -1].item()])
    g = H.check_loss_and_grads(D, shape, p, loss, grads, rloss, rgrads, both)
    touched = torch.unique(torch.cat([ids.reshape(-1), pos, neg])).cpu().numpy()
    rest = np.setdiff1d(np.arange(V), touched)
    assert not g[rest].any()                                  # exactly zero, every float written
    assert not rgrads["item_embeddings.weight"][rest].any()
    H.second_call_tail(D, m, shape, p, call, loss, grads)


def test_a_row_whose_answer_is_its_negative_adds_exactly_nothing():
    H.a_row_whose_answer_is_its_negative_adds_exactly_nothing(D)


@pytest.mark.parametrize("p,wd", [(0.0, 0.0), (0.5, 0.0), (0.5, 0.01)])
def test_three_train_steps_against_the_reference(p, wd):
    m = H.three_adam_steps(D, p, wd)
    flat = m.gru_layers._flat
    off = 0
    for k, q in m.named_parameters():
        if k != "item_embeddings.weight":                       # updated in place: still views of the flat array
            assert q.data_ptr() == flat.data_ptr() + 4 * off, k
            off += q.numel()
    assert off == flat.numel()


def test_determinism_with_a_poisoned_workspace():
    H.determinism_with_a_poisoned_workspace(D)


def test_graph_replay_is_the_next_step():
    H.graph_replay_is_the_next_step(D)


def test_main_run_with_the_fused_step(monkeypatch):
    H.main_run_with_the_fused_step(D, monkeypatch)


def test_trainer_mode_switch_and_checkpoint_round_trip(tmp_path):
    H.trainer_mode_switch_and_checkpoint_round_trip(D, tmp_path)
