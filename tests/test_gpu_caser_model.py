"""CaserModel on the GPU against the fp64 restatement (caser_ref.model_loss_grads): s, the BPR loss and every parameter gradient at
dropout 0 and at p > 0 (the mask recovered from the generator seed), three Adam steps against the same steps of a torch twin in
double on the CPU, the state_dict, the flat views after .cuda() / reflatten(), one Trainer epoch with the topk_full lists against
a dense ranking, and the Trainer's refusals.  (B, L, d) = (9, 12, 32), V = 50, n_h = 16, n_v = 4."""
import argparse
import functools

import numpy as np
import pytest

from conftest import rel_l2
import caser_ref as R

pytestmark = pytest.mark.gpu
OUT_GATE, GRAD_GATE = 2e-5, 2e-4
V, D, L, B, NH, NV = 50, 32, 12, 9, 16, 4
FZ = NV * D + NH * L


def _args(**kw):
    a = argparse.Namespace(item_size=V, hidden_size=D, max_seq_length=L, hidden_dropout_prob=0.0, initializer_range=0.02,
                           caser_nh=NH, caser_nv=NV, lr=1e-3, adam_beta1=0.9, adam_beta2=0.999, weight_decay=0.0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def _batch():
    import torch
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(1, V, (B, L), generator=g)
    ids[0, :7] = 0                                            # padding in front, not masked by this model: exact ties
    ids[1, :11] = 0
    ids[2, :] = 5
    pos = torch.randint(1, V, (B,), generator=g)
    neg = torch.randint(1, V, (B,), generator=g)
    pos[0], neg[1] = ids[0, -1], ids[1, -1]                   # rows of the table that the lookup and the head both touch
    return ids, pos, neg


@functools.lru_cache(maxsize=None)
def _model(p=0.0):
    """The model on the GPU with trained-size weights (a few times the init, so that s leaves 0 and the maxima spread) and its
    parameters as numpy arrays.  The seed is one at which the reference finds no ambiguous cell in the batch (caser_ref.ambiguous at
    1e-4; two cells at 1e-3): the whole-model gradients cannot mask one."""
    import torch
    from bsarec_amd import CaserModel
    torch.manual_seed(13)
    m = CaserModel(_args(hidden_dropout_prob=p))
    with torch.no_grad():
        m.item_embeddings.weight.mul_(40.0)
        m.fc1.weight.mul_(5.0)
        m.fc1.bias.normal_(0.0, 0.1)
    params = {k: v.detach().numpy().copy() for k, v in m.state_dict().items()}
    flat = m.conv._flat.detach().numpy().copy()
    return m.cuda(), params, flat


def _check(m, params, flat, keep, p):
    import torch
    ids, pos, neg = _batch()
    loss_r, s_r, g_r = R.model_loss_grads(params["item_embeddings.weight"], flat, params["fc1.weight"], params["fc1.bias"],
                                          ids.numpy(), pos.numpy(), neg.numpy(), NH, NV, keep, p)
    _, cache = R.forward(params["item_embeddings.weight"].astype(np.float64)[ids.numpy()], flat, NH, NV)
    assert not R.ambiguous(cache, 1e-4).any()                 # a condition on the inputs: no choice at fp32's rounding level
    m.zero_grad()
    loss = m.calculate_loss(ids.cuda(), pos.cuda(), neg.cuda())
    loss.backward()
    e_loss = abs(loss.item() - loss_r) / abs(loss_r)
    want = R.split_weights(g_r["conv"], L, D, NH, NV)
    errs = {}
    for k, q in m.named_parameters():
        ref = want[k[5:]] if k.startswith("conv.") else g_r[k]
        got = q.grad.cpu().numpy().reshape(ref.shape)
        if not ref.any():
            assert not got.any(), k                           # a bank none of whose cells passes: exactly zero
            continue
        errs[k] = rel_l2(got, ref)
    worst = max((v, k) for k, v in errs.items() if k.startswith("conv.conv_h"))
    print(f"caser model p={p}: loss {loss.item():.7f} rel {e_loss:.2e} E {errs['item_embeddings.weight']:.2e} "
          f"conv_v {errs['conv.conv_v.weight']:.2e} worst conv_h {worst[0]:.2e} ({worst[1]}) fc1 {errs['fc1.weight']:.2e}")
    assert e_loss <= 5e-6
    for k, v in errs.items():
        assert v <= GRAD_GATE, (k, v)
    touched = np.unique(np.concatenate([ids.numpy().reshape(-1), pos.numpy(), neg.numpy()]))
    g = m.item_embeddings.weight.grad.cpu().numpy()
    assert not g[np.setdiff1d(np.arange(V), touched)].any()
    return s_r


def test_state_loss_and_gradients_against_the_reference():
    import torch
    m, params, flat = _model()
    ids = _batch()[0].cuda()
    m.train()
    s_r = _check(m, params, flat, None, 0.0)
    m.eval()
    with torch.no_grad():
        s = m(ids)
        assert s.shape == (B, D)
        assert torch.equal(m.predict(ids), s) and torch.equal(m.last_hidden(ids), s)          # bit for bit
    m.train()
    assert torch.equal(m(ids).detach(), s)                    # p = 0; the train = 1 call gives the bits of train = 0
    e_s = rel_l2(s.cpu().numpy(), s_r)
    print(f"caser model: s {e_s:.2e}")
    assert e_s <= OUT_GATE and (s_r > 0).mean() > 0.2         # the ReLU is neither dead nor idle
    with pytest.raises(ValueError, match="max_seq_length"):
        m(ids[:, 1:])
    with pytest.raises(RuntimeError, match="MI355X"):
        m(ids.cpu())


def test_dropout_mask_is_recovered_from_the_seed():
    import torch
    p = 0.3
    m, params, flat = _model(p)
    m.train()
    m.set_seed(5)
    g = torch.Generator(device="cuda")
    g.manual_seed(5)
    keep = torch.empty(B, FZ, device="cuda").bernoulli_(1.0 - p, generator=g).cpu().numpy()
    assert 0.55 < keep.mean() < 0.85
    _check(m, params, flat, keep, p)
    ids = _batch()[0].cuda()
    with torch.no_grad():
        m.set_seed(5)
        a = m(ids)
        m.set_seed(5)
        b = m(ids)
        c = m(ids)                                            # the next draw of the same stream
        m.eval()
        e = m(ids)
    assert torch.equal(a, b) and not torch.equal(a, c) and not torch.equal(a, e)


def test_three_adam_steps_against_a_twin_in_double():
    import copy
    import torch
    from test_caser_cpu import Twin
    m0, params, _ = _model()
    m = copy.deepcopy(m0)
    m.conv.reflatten()
    m.train()
    twin = Twin(V, L, D, NH, NV).double()
    twin.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    ids, pos, neg = _batch()

    def twin_loss():
        E = twin.item_embeddings
        s = torch.relu(twin.fc1(twin.conv(E(ids))))
        return -torch.log(torch.sigmoid((s * E(pos)).sum(-1) - (s * E(neg)).sum(-1)) + 1e-10).mean()
    om = torch.optim.Adam(m.parameters(), lr=1e-3)
    ot = torch.optim.Adam(twin.parameters(), lr=1e-3)
    for _ in range(3):
        om.zero_grad()
        m.calculate_loss(ids.cuda(), pos.cuda(), neg.cuda()).backward()
        om.step()
        ot.zero_grad()
        twin_loss().backward()
        ot.step()
    flat = m.conv._flat
    lay = {"conv." + n: o for n, o, _ in R.layout(L, D, NH, NV)[0]}
    before = dict(m0.named_parameters())
    for (k, q), (k2, t) in zip(m.named_parameters(), twin.named_parameters()):
        assert k == k2
        e = rel_l2(q.detach().cpu().numpy(), t.detach().numpy())
        assert e <= 2e-4, (k, e)
        if k in lay:                                          # updated in place: still views of the flat array
            assert q.data_ptr() == flat.data_ptr() + 4 * lay[k], k
    assert not torch.equal(m.fc1.weight.detach().cpu(), before["fc1.weight"].detach().cpu())       # it moved
    assert not torch.equal(m.conv.conv_h[3].weight.detach().cpu(), before["conv.conv_h.3.weight"].detach().cpu())


def test_state_dict_and_views_after_cuda_and_reflatten():
    import torch
    from bsarec_amd import CaserModel
    torch.manual_seed(1)
    m = CaserModel(_args())
    keys = ["item_embeddings.weight", "conv.conv_v.weight", "conv.conv_v.bias"]
    for i in range(L):
        keys += [f"conv.conv_h.{i}.weight", f"conv.conv_h.{i}.bias"]
    keys += ["fc1.weight", "fc1.bias"]
    assert list(m.state_dict()) == keys
    cpu = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.cuda()
    assert list(m.state_dict()) == keys
    lay, total = R.layout(L, D, NH, NV)
    for step in range(2):
        flat = m.conv._flat
        assert flat.is_cuda and flat.numel() == total and flat.data_ptr() % 16 == 0
        ps = dict(m.named_parameters())
        covered = torch.zeros(total, dtype=torch.bool)
        for name, off, shp in lay:
            q = ps["conv." + name]
            assert q.data_ptr() == flat.data_ptr() + 4 * off and tuple(q.shape) == caser_shape(name, shp), name
            assert torch.equal(q.detach().cpu(), cpu["conv." + name])
            covered[off:off + q.numel()] = True
        assert not flat.cpu()[~covered].any()                 # the gaps hold zeros
        with torch.no_grad():                                 # give one parameter a storage of its own: reflatten() takes it back
            m.conv.conv_h[2].weight.data = m.conv.conv_h[2].weight.data.clone()
        assert m.conv.conv_h[2].weight.data_ptr() != flat.data_ptr() + 4 * dict((n, o) for n, o, _ in lay)["conv_h.2.weight"]
        m.conv.reflatten()
        assert m.conv._flat is not flat
    # the kernels read the array the views alias: an in-place change of a filter changes z
    x = torch.randn(2, L, D, device="cuda")
    with torch.no_grad():
        z0 = m.conv(x)
        m.conv.conv_v.bias.add_(1.0)
        z1 = m.conv(x)
    assert torch.allclose(z1[:, :NV * D], z0[:, :NV * D] + 1.0, atol=1e-5) and torch.equal(z1[:, NV * D:], z0[:, NV * D:])


def caser_shape(name, shp):
    """torch's Conv2d shape of a tensor of the flat array."""
    if name.endswith("bias"):
        return tuple(shp)
    return (shp[0], 1, shp[1], 1) if name == "conv_v.weight" else (shp[0], 1, shp[1], shp[2])


def _setup(argv):
    """What main.run builds before its epoch loop, for a Caser run on 120 users and 200 items."""
    import scipy.sparse as sp
    import torch
    from bsarec_amd import data as Dm, main as M
    from bsarec_amd.trainer import Trainer
    seqs = Dm.synth_ml1m_like(seed=5, n_users=120, n_items=200)
    args = M.parse_args(["--model_type", "Caser", "--max_seq_length", str(L), "--hidden_size", str(D), "--batch_size", "64",
                         "--epochs", "1", "--patience", "100"] + argv)
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


def test_trainer_epoch_and_topk_full_against_a_dense_ranking():
    import torch
    seqs, args, model, tr = _setup(["--caser_nh", "8", "--caser_nv", "2"])
    assert model.conv.n_h == 8 and model.conv.n_v == 2
    before = {k: v.detach().clone() for k, v in model.state_dict().items()}
    post = tr.train(0)
    assert np.isfinite(float(post["rec_loss"]))
    for k in ("item_embeddings.weight", "conv.conv_v.weight", "conv.conv_v.bias", "conv.conv_h.0.weight", "conv.conv_h.5.bias",
              "fc1.weight", "fc1.bias"):
        assert not torch.equal(model.state_dict()[k], before[k]), k                           # the optimiser walks the views
    scores, _ = tr.test(0)
    assert len(scores) == 6 and np.isfinite(scores).all() and all(0.0 <= s <= 1.0 for s in scores)
    args.eval_full_rank = "fused"
    assert list(tr.test(0)[0]) == list(scores)                # no full_logits: the default path is topk_full already
    # one batch: the lists against s @ E^T in double with the seen items' scores set to 0 (the reference's rule), ties to the
    # smaller id; a position may differ only where the two candidates' scores agree to fp32 rounding
    args.train_matrix = args.test_rating_matrix
    users, ids = next(iter(tr.test_dataloader))[:2]
    k = 20
    pred = tr.topk_full(users, ids, k=k).cpu().numpy()
    s = model.last_hidden(ids).double().cpu().numpy()
    dense = s @ model.item_embeddings.weight.detach().double().cpu().numpy().T
    csr = args.test_rating_matrix.tocsr()
    for r, u in enumerate(users.cpu().numpy()):
        dense[r, csr.indices[csr.indptr[u]:csr.indptr[u + 1]]] = 0.0
    tol = 4e-6 * np.abs(dense).max()
    exact = 0
    for r in range(dense.shape[0]):
        order = np.lexsort((np.arange(dense.shape[1]), -dense[r]))[:k]
        assert len(set(pred[r])) == k
        assert np.abs(dense[r, pred[r]] - dense[r, order]).max() <= tol
        exact += int(np.array_equal(pred[r], order))
    assert exact >= 0.9 * dense.shape[0]                      # the lists themselves, wherever no two scores are that close


def test_trainer_refusals_name_the_model():
    from bsarec_amd import CaserModel, GRU4RecModel
    from bsarec_amd.trainer import Trainer
    m = CaserModel(_args())
    with pytest.raises(ValueError, match="^Caser: single GPU only$"):
        Trainer(m, None, None, None, _args(), process_group=object())
    for k, v, msg in (("train_negatives", 8, "Caser: train_negatives does not apply"),
                      ("train_lazy_adam", True, "Caser: train_lazy_adam does not apply"),
                      ("storage", "bf16", "Caser: storage = 'bf16' does not apply \\(the Caser kernels are fp32\\)")):
        with pytest.raises(ValueError, match="^" + msg):
            Trainer(m, None, None, None, _args(**{k: v}))
    g = GRU4RecModel(argparse.Namespace(item_size=V, hidden_size=D, num_hidden_layers=1, max_seq_length=L, hidden_dropout_prob=0.0,
                                        initializer_range=0.02))
    with pytest.raises(ValueError) as e:
        Trainer(g, None, None, None, _args(), process_group=object())
    assert str(e.value) == "GRU4Rec: single GPU only"
    with pytest.raises(ValueError) as e:
        Trainer(g, None, None, None, _args(storage="bf16"))
    assert str(e.value) == "GRU4Rec: storage = 'bf16' does not apply (the GRU kernels are fp32)"
    with pytest.raises(ValueError) as e:
        Trainer(g, None, None, None, _args(train_negatives=8))
    assert str(e.value) == "GRU4Rec: train_negatives does not apply (the model has its own BPR head)"
    with pytest.raises(ValueError) as e:
        Trainer(g, None, None, None, _args(train_lazy_adam=True))
    assert str(e.value) == "GRU4Rec: train_lazy_adam does not apply (the model steps through torch.optim.Adam)"
