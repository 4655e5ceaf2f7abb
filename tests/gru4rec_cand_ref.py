"""The GRU4Rec heads over candidates shared by the batch (bsarec_gru4rec_cand_head, include/bsarec_hip.h) in numpy double, and the
whole step with them: gru4rec_step_ref's gather, mask, GRU stack and Adam around ``head`` in place of the pairwise BPR rows.

The candidates: ``negatives = "in_batch"``: C = B, c_j = answers[j]; ``"in_batch+sampled"``: C = 2 B, the answers and then
neg_answers.  r = s . E[c]^T; row b's positive is column b, its negatives M_b = {j : c_j != answers[b]}, m_b = |M_b|; a row with
m_b = 0 has loss 0 and gradient 0; loss = mean_b loss_b:
  ce       loss_b = logsumexp_{{b} + M_b} r_bj - r_bb
  top1     loss_b = (1 / m_b) sum_{M_b} [sig(r_bj - r_bb) + sig(r_bj^2)]
  bpr_max  p = softmax over M_b, A = sum p_j sig(r_bb - r_bj), Q = sum p_j r_bj^2, loss_b = -log(A + 1e-10) + bpreg Q"""
import numpy as np

import gru_ref as R
import gru4rec_step_ref as S

LOSSES = ("ce", "top1", "bpr_max")
NEGATIVES = ("in_batch", "in_batch+sampled")
EPS = 1e-10


def sigmoid(x):
    """Formed from e^{-|x|}: no overflow, 0 or 1 exactly for large |x|."""
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def candidates(pos, neg, negatives):
    pos, neg = np.asarray(pos, np.int64).reshape(-1), np.asarray(neg, np.int64).reshape(-1)
    return pos if negatives == "in_batch" else np.concatenate([pos, neg])


def negative_mask(pos, neg, negatives):
    """[B, C] bool: column j is a negative of row b."""
    pos = np.asarray(pos, np.int64).reshape(-1)
    return candidates(pos, neg, negatives)[None, :] != pos[:, None]


def head(s, E, pos, neg, loss, negatives, bpreg=1.0):
    """-> (loss, G [B, C] = d(loss) / d(r), ds [B, d] = G . E_c, dEc [C, d] = G^T . s)."""
    s, E = np.asarray(s, np.float64), np.asarray(E, np.float64)
    Ec = E[candidates(pos, neg, negatives)]
    B = s.shape[0]
    r = s @ Ec.T
    M = negative_mask(pos, neg, negatives)
    G = np.zeros_like(r)
    rows = np.zeros(B)
    for b in range(B):
        j = np.flatnonzero(M[b])
        m = j.size
        if m == 0:
            continue
        x, xb = r[b, j], r[b, b]
        if loss == "ce":
            a = np.concatenate([[xb], x])
            mx = a.max()
            e = np.exp(a - mx)
            rows[b] = mx + np.log(e.sum()) - xb
            p = e / e.sum()
            G[b, j] = p[1:]
            G[b, b] = p[0] - 1.0
        elif loss == "top1":
            sg, sq = sigmoid(x - xb), sigmoid(x * x)
            u = sg * (1.0 - sg)
            rows[b] = (sg + sq).sum() / m
            G[b, j] = (u + 2.0 * x * sq * (1.0 - sq)) / m
            G[b, b] = -u.sum() / m
        elif loss == "bpr_max":
            e = np.exp(x - x.max())
            p = e / e.sum()
            sg = sigmoid(xb - x)
            u = sg * (1.0 - sg)
            A, Q = (p * sg).sum(), (p * x * x).sum()
            rows[b] = -np.log(A + EPS) + bpreg * Q
            G[b, j] = -(p * (sg - A) - p * u) / (A + EPS) + bpreg * (p * (x * x - Q) + 2.0 * p * x)
            G[b, b] = -(p * u).sum() / (A + EPS)
        else:
            raise ValueError(loss)
    G /= B
    return float(rows.mean()), G, G @ Ec, G.T @ s


def loss_and_grads(params, ids, pos, neg, H, N, loss, negatives, bpreg=1.0, mult=None):
    """gru4rec_step_ref.loss_and_grads with the candidate head: -> (loss, {key: gradient})."""
    E = np.asarray(params["item_embeddings.weight"], np.float64)
    ids, pos, neg = (np.asarray(v, np.int64) for v in (ids, pos, neg))
    B, L = ids.shape
    d = E.shape[1]
    mult = np.ones((B, L, d)) if mult is None else np.asarray(mult, np.float64)
    out, cache = R.forward(E[ids] * mult, S.flat_of(params, N), H, N, d)
    val, _, ds, dEc = head(out[:, L - 1], E, pos, neg, loss, negatives, bpreg)
    dx, dflat = R.backward(cache, R.last_only_dout(ds, L))
    dE = np.zeros_like(E)
    np.add.at(dE, ids.reshape(-1), (dx * mult).reshape(-1, d))
    np.add.at(dE, candidates(pos, neg, negatives), dEc)
    grads = {"item_embeddings.weight": dE}
    for name, g in R.split_weights(dflat, d, H, N, d).items():
        grads[S.GRU_NAMES.get(name, "gru_layers." + name)] = g
    return val, {k: grads[k] for k in S.keys(N)}


def train_step(params, st, ids, pos, neg, H, N, loss, negatives, bpreg=1.0, mult=None):
    """One step in place: the gradients at ``params``, then oracle.adam_step.  Returns the loss."""
    val, grads = loss_and_grads(params, ids, pos, neg, H, N, loss, negatives, bpreg, mult)
    S.O.adam_step(params, grads, st)
    return val
