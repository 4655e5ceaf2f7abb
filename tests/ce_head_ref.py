"""fp64 numpy restatement of bsarec_ce_head_fwd / bsarec_ce_head_bwd (include/bsarec_hip.h): the full-catalogue cross-entropy of
a hidden state, its rows, and the gradients with respect to the hidden state and the item table."""
import numpy as np


def ce_head(h, E, answers, g=1.0):
    """h [B, d], E [V, d], answers [B] (clamped to [0, V)), upstream scalar g -> (loss, rows [B], dh [B, d], dE [V, d])."""
    h, E = np.asarray(h, np.float64), np.asarray(E, np.float64)
    B, V = h.shape[0], E.shape[0]
    a = np.clip(np.asarray(answers, np.int64), 0, V - 1)
    s = h @ E.T
    m = s.max(axis=1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(s - m).sum(axis=1))
    rows = lse - s[np.arange(B), a]
    G = np.exp(s - lse[:, None])
    G[np.arange(B), a] -= 1.0
    G *= g / B
    return rows.mean(), rows, G @ E, G.T @ h
