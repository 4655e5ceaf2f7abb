"""The fused Caser step on the GPU (caser_step = "fused": bsarec_caser_loss_grad / bsarec_caser_train_step) against the step in
numpy double (caser_step_ref): loss and every gradient at p = 0 and p = 0.5 on three shapes, three Adam steps, bit determinism
with a poisoned workspace, graph replay against eager calls, and the trainer end to end.

  shape 1  V = 301, d = 64, L = 12, B = 17, n_h = 16, n_v = 4   204 tokens: no multiple of the scatter chunk; F = 448
  shape 2  V = 5, d = 36, L = 1, B = 17, n_h = 4, n_v = 1       d no multiple of 16, L = 1, every row of the table hit many times
  shape 3  V = 40, d = 256, L = 3, B = 65, n_h = 32, n_v = 16   the widest rows, F = 4192

The whole step cannot zero the dz of a cell, so the inputs must leave fp32 no discrete choice to get wrong: at every set of weights
a test visits (the three Adam steps included) the reference marks NO ambiguous convolution cell (caser_ref.ambiguous at 1e-4) and
no pre-activation of fc1 has |u| < 1e-4.  That is a condition on the inputs, asserted from the reference; the model seeds below
were found by a search on the CPU: the first seed from 0 at which the condition holds at the initial weights under both masks
and, at shape 1, at the seven sets of weights of the three-step cases.  Shape 1 was meant to have B = 33: no seed in 0 .. 199 holds
over the three steps there, nor at B = 17, where the first that does is 5629 (every Adam step moves every filter by about lr, so
each set of weights is a fresh draw of 3,264 cells against the margin); so shape 1 has B = 17, one row past a 16-row tile."""
import argparse

import numpy as np
import pytest

from conftest import rel_l2
import caser_ref as R
import caser_step_ref as S
import step_harness as H

pytestmark = pytest.mark.gpu
LOSS_GATE, OUT_GATE, GRAD_GATE = 5e-6, 2e-5, 2e-4
MARGIN = 1e-4
SHAPES = {1: (301, 64, 12, 17, 16, 4), 2: (5, 36, 1, 17, 4, 1), 3: (40, 256, 3, 65, 32, 16)}     # V, d, L, B, n_h, n_v
MODEL_SEED = {1: 5629, 2: 0, 3: 13}
SEED = 5
STEP_CASES = [(0.0, 0.0), (0.5, 0.0), (0.5, 0.01)]                                               # (p, weight decay)


def _args(shape, p=0.0, **kw):
    V, d, L, B, nh, nv = SHAPES[shape]
    a = argparse.Namespace(item_size=V, hidden_size=d, max_seq_length=L, hidden_dropout_prob=p, initializer_range=0.02,
                           caser_nh=nh, caser_nv=nv, lr=1e-3, adam_beta1=0.9, adam_beta2=0.999, weight_decay=0.0,
                           caser_step="fused")
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _batch(shape):
    V, d, L, B, nh, nv = SHAPES[shape]
    return H.pairwise_batch(V, L, B)


def _host_model(shape, p=0.0, seed=None, **kw):
    """A fused-step model on the CPU with trained-size weights, scaled as test_gpu_caser_model._model does (E ~ N(0, 0.8),
    fc1 ~ N(0, 0.1)); the same weights for every p and option."""
    import torch
    from bsarec_amd import CaserModel
    torch.manual_seed(MODEL_SEED[shape] if seed is None else seed)
    m = CaserModel(_args(shape, p, **kw))
    with torch.no_grad():
        m.item_embeddings.weight.mul_(40.0)
        m.fc1.weight.mul_(5.0)
        m.fc1.bias.normal_(0.0, 0.1)
    return m


def _model(shape, p=0.0, **kw):
    m = _host_model(shape, p, **kw).cuda()
    m.train()
    m.set_seed(SEED)
    return m


def _mult(shape, p, seed, step):
    V, d, L, B, nh, nv = SHAPES[shape]
    return S.dropout_mult(B, nv * d + nh * L, p, seed, step)


def _assert_condition(params, ids, mult, what):
    cells, umin = S.condition(params, ids, mult, MARGIN)
    assert cells == 0 and umin >= MARGIN, (what, cells, umin)             # a condition on the inputs, not a tolerance


def _reference(shape, p, seed, step):
    """Loss, s and gradients of the reference at the model's initial weights, under the mask of (seed, step)."""
    ids, pos, neg = H.host(D, shape)
    params = H.params64(_host_model(shape))
    mult = _mult(shape, p, seed, step)
    _assert_condition(params, ids, mult, (shape, p))
    return S.loss_and_grads(params, ids, pos, neg, mult)


D = H.describe(stem="caser", name="Caser", flag="caser_step", seed=SEED, loss_gate=LOSS_GATE, grad_gate=GRAD_GATE,
               vbl=lambda shape: (SHAPES[shape][0], SHAPES[shape][3], SHAPES[shape][2]), slot=lambda B, L: B,
               args=_args, model=_model, batch=_batch, reference=_reference, mults=_mult,
               train_step=lambda params, st, hb, mult: S.train_step(params, st, *hb, mult),
               before_step=lambda params, hb, mult, what: _assert_condition(params, hb[0], mult, what),
               eval_kw=dict(train=False),
               adam_tag="caser fused adam",
               moved=("item_embeddings.weight", "conv.conv_v.weight", "conv.conv_v.bias", "conv.conv_h.0.weight",
                      "conv.conv_h.5.bias", "fc1.weight", "fc1.bias"),
               main=dict(argv=["--max_seq_length", "12", "--hidden_size", "32", "--batch_size", "64"],
                         synth=dict(n_users=120, n_items=200), tag="fused caser main.run"),
               trainer=("test_gpu_caser_model", "fc1.weight"))


def _line(errs):
    worst = max((v, k) for k, v in errs.items() if k.startswith("conv.conv_h"))
    return (f"E {errs['item_embeddings.weight']:.2e} conv_v {errs['conv.conv_v.weight']:.2e} / {errs['conv.conv_v.bias']:.2e} "
            f"worst conv_h {worst[0]:.2e} ({worst[1]}) fc1 {errs['fc1.weight']:.2e} / {errs['fc1.bias']:.2e}")


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("shape", [1, 2, 3])
def test_loss_and_grads_against_the_reference(shape, p):
    import torch
    V, d, L, B, nh, nv = SHAPES[shape]
    m, call, loss, grads, (rloss, _, rgrads) = H.first_call(D, shape, p)
    ids, pos, neg = call[0]
    assert list(grads) == list(m.state_dict()) == S.keys(L)
    both = np.array([ids[6, -1].item(), ids[7, -1].item()])
    g = H.check_loss_and_grads(D, shape, p, loss, grads, rloss, rgrads, both, zero_banks=True, line=_line)
    touched = torch.unique(torch.cat([ids.reshape(-1), pos, neg])).cpu().numpy()
    rest = np.setdiff1d(np.arange(V), touched)
    assert not g[rest].any()                                  # exactly zero, every float written
    assert not rgrads["item_embeddings.weight"][rest].any()
    H.second_call_tail(D, m, shape, p, call, loss, grads)


def test_state_of_the_step_against_the_reference():
    """s as the step forms it (read from the step's workspace region) at p = 0.5, and forward() in eval mode at p = 0."""
    import torch
    V, d, L, B, nh, nv = SHAPES[1]
    (ids, pos, neg), _ = H.cuda(D, 1)
    m = _model(1, 0.0)
    m.eval()
    with torch.no_grad():
        s = m(ids)
    m.train()
    e0 = rel_l2(s.cpu().numpy(), H.reference(D, 1, 0.0, SEED, 1)[1])
    assert e0 <= OUT_GATE
    m = _model(1, 0.5)
    m.loss_and_grads(ids, pos, neg, train=True)
    F = nv * d + nh * L
    slot = m._fused["slots"][B]
    conv_floats = B * L * nh                                  # the convolution workspace of train = 1, a multiple of 4 ints
    off = conv_floats + B * L * d + 2 * B * F                 # | x | z | zd | s
    s5 = slot["ws"].view(torch.float32)[off:off + B * d].view(B, d).cpu().numpy()
    s_r = H.reference(D, 1, 0.5, SEED, 1)[1]
    e5 = rel_l2(s5, s_r)
    print(f"caser step s: p=0 {e0:.2e} p=0.5 {e5:.2e} alive {(s_r > 0).mean():.2f}")
    assert e5 <= OUT_GATE and (s_r > 0).mean() > 0.2          # the ReLU is neither dead nor idle


def test_a_row_whose_answer_is_its_negative_adds_exactly_nothing():
    H.a_row_whose_answer_is_its_negative_adds_exactly_nothing(D)


@pytest.mark.parametrize("p,wd", STEP_CASES)
def test_three_train_steps_against_the_reference(p, wd):
    V, d, L, B, nh, nv = SHAPES[1]
    m = H.three_adam_steps(D, p, wd)
    flat, fc = m.conv._flat, m._fc_flat
    lay = {"conv." + n: o for n, o, _ in R.layout(L, d, nh, nv)[0]}
    for k, q in m.named_parameters():
        if k in lay:                                          # updated in place: still views of the flat arrays
            assert q.data_ptr() == flat.data_ptr() + 4 * lay[k], k
    assert m.fc1.weight.data_ptr() == fc.data_ptr() and m.fc1.bias.data_ptr() == fc.data_ptr() + 4 * m.fc1.weight.numel()
    assert fc.numel() == m.fc1.weight.numel() + d


def test_determinism_with_a_poisoned_workspace():
    H.determinism_with_a_poisoned_workspace(D)


def test_graph_replay_is_the_next_step():
    H.graph_replay_is_the_next_step(D)


def test_main_run_with_the_fused_step(monkeypatch):
    H.main_run_with_the_fused_step(D, monkeypatch)


def test_trainer_mode_switch_and_checkpoint_round_trip(tmp_path):
    H.trainer_mode_switch_and_checkpoint_round_trip(D, tmp_path)
