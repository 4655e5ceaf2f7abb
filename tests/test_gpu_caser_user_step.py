"""The fused step of the personalised Caser on the GPU (caser_user with caser_step = "fused": bsarec_caser_user_loss_grad /
bsarec_caser_user_train_step) against the step in numpy double (caser_user_ref): loss, z1 / x2 / s out of the workspace and every
gradient at p = 0 and p = 0.5 on four shapes, the exact properties of the user half, three Adam steps, bit determinism with a
poisoned workspace, graph replay against eager calls, and a replay after the users changed.

  shape 1  V = 301, U = 7,  d = 64,  L = 12, B = 17, n_h = 16, n_v = 4   a row-tile tail; 17 rows over 7 users: duplicates
  shape 2  V = 5,   U = 1,  d = 36,  L = 1,  B = 17, n_h = 4,  n_v = 1   d no multiple of 16, every row on one user, L = 1
  shape 3  V = 40,  U = 70, d = 256, L = 3,  B = 65, n_h = 32, n_v = 16  K = 512 in fc2, 16 column tiles, untouched user rows
  shape 4  V = 9,   U = 3,  d = 4,   L = 2,  B = 1,  n_h = 4,  n_v = 1   the minimum d and B

No element or row is left out of a comparison, so the inputs must leave fp32 no discrete choice to get wrong: at every set of
weights a test visits (the three Adam steps included) the reference marks NO ambiguous convolution cell (caser_ref.ambiguous at
1e-4) and no pre-activation of fc1 or of fc2 has |u| < 1e-4.  That is a condition on the inputs, asserted from the reference; the
model seeds below were found by a search on the CPU over the fp64 reference: the first seed from 0 at which the condition holds at
the initial weights under both masks (at shape 2 also with the out-of-range users of its own test) and, at shape 1, at the seven
sets of weights of the three-step cases (shape 1: 1092; 286 seeds below it hold at the initial weights and fail at a later set).
At shape 4 seed 0 holds too, but its bank of height 2 passes nothing: seed 1 is the first at which, besides, every gradient
tensor of the reference is non-zero."""
import argparse

import numpy as np
import pytest

from conftest import rel_l2
import caser_ref as R
import caser_user_ref as UR
import step_harness as H

pytestmark = pytest.mark.gpu
LOSS_GATE, OUT_GATE, GRAD_GATE = 5e-6, 2e-5, 2e-4
MARGIN = 1e-4
SHAPES = {1: (301, 7, 64, 12, 17, 16, 4), 2: (5, 1, 36, 1, 17, 4, 1), 3: (40, 70, 256, 3, 65, 32, 16),
          4: (9, 3, 4, 2, 1, 4, 1)}                                                              # V, U, d, L, B, n_h, n_v
MODEL_SEED = {1: 1092, 2: 0, 3: 3, 4: 1}
SEED = 5
STEP_CASES = [(0.0, 0.0), (0.5, 0.0), (0.5, 0.01)]                                               # (p, weight decay)


def _args(shape, p=0.0, **kw):
    V, U, d, L, B, nh, nv = SHAPES[shape]
    a = argparse.Namespace(item_size=V, num_users=U, hidden_size=d, max_seq_length=L, hidden_dropout_prob=p,
                           initializer_range=0.02, caser_nh=nh, caser_nv=nv, lr=1e-3, adam_beta1=0.9, adam_beta2=0.999,
                           weight_decay=0.0, caser_step="fused", caser_user=True)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _batch(shape):
    """The pairwise batch with users that include 0, U - 1 and repeats."""
    import torch
    V, U, d, L, B, nh, nv = SHAPES[shape]
    ids, users, pos, neg = H.pairwise_batch(V, L, B, U)
    if B > 10:
        users[0], users[1], users[2], users[5] = 0, U - 1, users[3], U - 1
        if U <= B - 6:
            users[6:6 + U] = torch.arange(U)                  # fewer users than rows: every one of them is named
    return ids, users, pos, neg


def _users_outside(shape):
    """The users of the batch with two rows outside [0, U): one at U, one negative."""
    users = H.batch(D, shape)[1].clone()
    users[3], users[11] = SHAPES[shape][1], -1
    return users


def _host_model(shape, p=0.0, seed=None, **kw):
    """A fused-step model on the CPU with trained-size weights, scaled as test_gpu_caser_step._host_model does (E, P ~ N(0, 0.8),
    fc1, fc2 ~ N(0, 0.1), biases N(0, 0.1)); the same weights for every p and option."""
    import torch
    from bsarec_amd import CaserModel
    torch.manual_seed(MODEL_SEED[shape] if seed is None else seed)
    m = CaserModel(_args(shape, p, **kw))
    with torch.no_grad():
        m.item_embeddings.weight.mul_(40.0)
        m.user_embeddings.weight.mul_(40.0)
        m.fc1.weight.mul_(5.0)
        m.fc1.bias.normal_(0.0, 0.1)
        m.fc2.weight.mul_(5.0)
        m.fc2.bias.normal_(0.0, 0.1)
    return m


def _model(shape, p=0.0, **kw):
    m = _host_model(shape, p, **kw).cuda()
    m.train()
    m.set_seed(SEED)
    return m


def _mult(shape, p, seed, step):
    V, U, d, L, B, nh, nv = SHAPES[shape]
    return UR.dropout_mult(B, nv * d + nh * L, p, seed, step)


def _assert_condition(params, ids, users, mult, what):
    cells, umin = UR.condition(params, ids, users, mult, MARGIN)
    assert cells == 0 and umin >= MARGIN, (what, cells, umin)             # a condition on the inputs, not a tolerance


def _reference(shape, p, seed, step, outside=False):
    """Loss, (z1, x2, s) and gradients of the reference at the model's initial weights, under the mask of (seed, step)."""
    ids, users, pos, neg = H.host(D, shape)
    if outside:
        users = _users_outside(shape).numpy()
    params = H.params64(_host_model(shape))
    mult = _mult(shape, p, seed, step)
    _assert_condition(params, ids, users, mult, (shape, p, outside))
    return UR.loss_and_grads(params, ids, users, pos, neg, mult)


def _call(batch):
    ids, users, pos, neg = batch
    return (ids, pos, neg), dict(user_ids=users)


D = H.describe(stem="caser_user", name="Caser", flag="caser_step", seed=SEED, loss_gate=LOSS_GATE,
               grad_gate=GRAD_GATE, vbl=lambda shape: (SHAPES[shape][0], SHAPES[shape][4], SHAPES[shape][3]), slot=lambda B, L: B,
               args=_args, model=_model, batch=_batch, reference=_reference, mults=_mult, call=_call,
               train_step=lambda params, st, hb, mult: UR.train_step(params, st, *hb, mult),
               before_step=lambda params, hb, mult, what: _assert_condition(params, hb[0], hb[1], mult, what),
               eval_kw=dict(train=False), adam_tag="caser user fused adam",
               moved=("item_embeddings.weight", "user_embeddings.weight", "conv.conv_v.weight", "conv.conv_h.0.weight",
                      "conv.conv_h.5.bias", "fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"))


def _workspace_regions(m, shape):
    """z1, x2 and s of the last call, read out of the step's workspace by the layout the header documents."""
    import torch
    from bsarec_amd import _lib
    V, U, d, L, B, nh, nv = SHAPES[shape]
    F, T = nv * d + nh * L, B * L
    slot = m._fused["slots"][B]
    conv_bytes = _lib.load().bsarec_caser_workspace_bytes(slot["cfg"].step.conv, 1)
    assert conv_bytes > 0 and conv_bytes % 16 == 0
    w = slot["ws"].view(torch.float32)
    z1_at = conv_bytes // 4 + T * d + 2 * B * F                           # conv | x | z | zd | s = z1
    item_only = z1_at + 2 * B * d + B * F + T * d + 2 * ((B + 3) // 4 * 4) + 2 * V * d     # ... | ds | dz | dx | c | rows | acc
    assert 4 * item_only == _lib.load().bsarec_caser_step_workspace_bytes(slot["cfg"].step)
    assert 4 * (item_only + 6 * B * d + 2 * U * d) == slot["nbytes"]
    z1 = w[z1_at:z1_at + B * d].view(B, d)
    x2 = w[item_only:item_only + 2 * B * d].view(B, 2 * d)
    s = w[item_only + 2 * B * d:item_only + 3 * B * d].view(B, d)
    return z1.clone(), x2.clone(), s.clone()


def _compare(shape, p, m, users, loss, grads, ref, tag):
    """Loss, workspace regions and every gradient against the reference; the exact properties of the user half."""
    import torch
    V, U, d, L, B, nh, nv = SHAPES[shape]
    rloss, rout, rgrads = ref
    assert list(grads) == list(m.state_dict()) == UR.keys(L)
    e_loss = abs(loss.item() - rloss) / abs(rloss)
    z1, x2, s = _workspace_regions(m, shape)
    e_out = {k: rel_l2(v.cpu().numpy(), rout[k]) for k, v in (("z1", z1), ("x2", x2), ("s", s))}
    errs = {}
    for k, g in grads.items():
        if not rgrads[k].any():
            assert not g.any().item(), k                      # a bank none of whose cells passes: exactly zero
            continue
        errs[k] = rel_l2(g.cpu().numpy(), rgrads[k])
    worst = max([(v, k) for k, v in errs.items() if k.startswith("conv.conv_h")], default=(0.0, None))
    e = {k.replace(".weight", ""): v for k, v in errs.items()}            # an all-zero gradient has no entry: printed as nan
    nan = float("nan")
    print(f"caser user step {tag} shape {shape} p={p}: loss {loss.item():.7f} rel {e_loss:.2e} z1 {e_out['z1']:.2e} "
          f"x2 {e_out['x2']:.2e} s {e_out['s']:.2e} alive {(rout['s'] > 0).mean():.2f} / {(rout['z1'] > 0).mean():.2f} "
          f"E {e.get('item_embeddings', nan):.2e} P {e.get('user_embeddings', nan):.2e} "
          f"conv_v {e.get('conv.conv_v', nan):.2e} worst conv_h {worst[0]:.2e} ({worst[1]}) "
          f"fc1 {e.get('fc1', nan):.2e} / {e.get('fc1.bias', nan):.2e} fc2 {e.get('fc2', nan):.2e} / {e.get('fc2.bias', nan):.2e}")
    assert (rout["s"] > 0).any() and (rout["z1"] > 0).any()              # neither ReLU is dead on these inputs
    assert e_loss <= LOSS_GATE
    for k, v in e_out.items():
        assert v <= OUT_GATE, (k, v)
    for k, v in errs.items():
        assert v <= GRAD_GATE, (k, v)
    # the user half: the table's rows bit for bit (zeros for an id outside the table), z1 copied bit for bit
    P = m.user_embeddings.weight.detach()
    inside = (users >= 0) & (users < U)
    want = P[users.clamp(0, U - 1)] * inside.unsqueeze(-1)
    assert torch.equal(x2[:, d:], want) and torch.equal(x2[:, :d], z1)
    # rows of the user table that no row of the batch names: exactly zero, every float written
    named = torch.unique(users[inside]).cpu().numpy()
    rest = np.setdiff1d(np.arange(U), named)
    gP = grads["user_embeddings.weight"].cpu().numpy()
    assert not gP[rest].any() and not rgrads["user_embeddings.weight"][rest].any()
    return rest


@pytest.mark.parametrize("p", [0.0, 0.5])
@pytest.mark.parametrize("shape", [1, 2, 3, 4])
def test_loss_and_grads_against_the_reference(shape, p):
    import torch
    V, U, d, L, B, nh, nv = SHAPES[shape]
    m, call, loss, grads, ref = H.first_call(D, shape, p)
    (ids, pos, neg), users = call[0], call[1]["user_ids"]
    if shape < 4:
        assert (users == 0).any() and (users == U - 1).any() and len(torch.unique(users)) < B
    rest = _compare(shape, p, m, users, loss, grads, ref, "grads")
    assert (len(rest) > 0) == (shape in (3, 4))               # more users than rows: untouched rows exist there
    touched = torch.unique(torch.cat([ids.reshape(-1), pos, neg])).cpu().numpy()
    gE = grads["item_embeddings.weight"].cpu().numpy()
    assert not gE[np.setdiff1d(np.arange(V), touched)].any()
    # [B, 1] user ids are the same call
    H.second_call_tail(D, m, shape, p, call, loss, grads, again=dict(user_ids=users.view(B, 1)))


def test_a_user_id_outside_the_table_gives_a_zero_half_and_adds_nothing():
    import torch
    shape = 2
    V, U, d, L, B, nh, nv = SHAPES[shape]
    m = _model(shape, 0.5)
    (ids, pos, neg), _ = H.cuda(D, shape)
    users = _users_outside(shape).cuda()
    loss, grads = m.loss_and_grads(ids, pos, neg, train=True, user_ids=users)
    _compare(shape, 0.5, m, users, loss, grads, H.reference(D, shape, 0.5, SEED, 1, True), "outside")
    _, x2, _ = _workspace_regions(m, shape)
    assert not x2[[3, 11], d:].any().item() and x2[0, d:].any().item()
    # every user outside: the whole half is zero and the user table gets exactly no gradient
    m = _model(shape, 0.0)
    nobody = torch.full((B,), U + 5, dtype=torch.int64, device="cuda")
    nobody[::2] = -7
    _, grads = m.loss_and_grads(ids, pos, neg, train=False, user_ids=nobody)
    _, x2, _ = _workspace_regions(m, shape)
    assert not x2[:, d:].any().item() and not grads["user_embeddings.weight"].any().item()
    assert grads["fc2.weight"][:, :d].any().item() and not grads["fc2.weight"][:, d:].any().item()
    # the torch-op path of forward / last_hidden follows the same rule
    m.eval()
    with torch.no_grad():
        s_nobody = m(ids, nobody)
        P = m.user_embeddings.weight.detach().clone()
        m.user_embeddings.weight.zero_()
        s_zero = m(ids, torch.zeros(B, dtype=torch.int64, device="cuda"))
        m.user_embeddings.weight.copy_(P)
    assert torch.equal(s_nobody, s_zero)


@pytest.mark.parametrize("p,wd", STEP_CASES)
def test_three_train_steps_against_the_reference(p, wd):
    V, U, d, L, B, nh, nv = SHAPES[1]
    m = H.three_adam_steps(D, p, wd)
    flat, fc, fc2 = m.conv._flat, m._fc_flat, m._fc2_flat
    lay = {"conv." + n: o for n, o, _ in R.layout(L, d, nh, nv)[0]}
    for k, q in m.named_parameters():
        if k in lay:                                          # updated in place: still views of the flat arrays
            assert q.data_ptr() == flat.data_ptr() + 4 * lay[k], k
    assert m.fc1.weight.data_ptr() == fc.data_ptr() and m.fc1.bias.data_ptr() == fc.data_ptr() + 4 * m.fc1.weight.numel()
    assert m.fc2.weight.data_ptr() == fc2.data_ptr() and m.fc2.bias.data_ptr() == fc2.data_ptr() + 4 * m.fc2.weight.numel()
    assert fc2.numel() == 2 * d * d + d
    assert m.user_embeddings.weight.data_ptr() == m._fused["P"].data_ptr()


def test_determinism_with_a_poisoned_workspace():
    H.determinism_with_a_poisoned_workspace(D)


def test_graph_replay_is_the_next_step():
    H.graph_replay_is_the_next_step(D)


def test_a_replay_reads_the_users_of_its_own_step():
    import torch
    V, U, d, L, B, nh, nv = SHAPES[1]
    u0 = H.batch(D, 1)[1]
    u1 = (u0 + 3) % U                                             # other users in the static buffer for the second replay
    assert not torch.equal(u0, u1)
    a, _ = H.cuda(D, 1)
    lg, pg = H.graph_replay_is_the_next_step(D, calls=[(a, dict(user_ids=u.cuda())) for u in (u0, u1, u0)])
    ls, ps = H.three_steps(D, _model(1, 0.5))                      # the same users three times: another result
    assert torch.equal(ls[0], lg[0]) and not torch.equal(ls[1], lg[1])
    assert not torch.equal(ps["user_embeddings.weight"], pg["user_embeddings.weight"])
