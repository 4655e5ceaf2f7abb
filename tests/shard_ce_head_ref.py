"""fp64 numpy restatement of the range form of the full-catalogue CE head (bsarec_ce_head_range_stats / _merge / _bwd,
include/bsarec_hip.h), built on ce_head_ref: a catalogue of V rows cut into W contiguous ranges of ceil(V / W) rows, the last
ones shorter or empty, as ShardedCatalogue cuts it."""
import numpy as np


def ranges(V, W):
    """[(col_base, Vs)] of the W ranks; a rank behind the last row owns the empty range [V, V)."""
    per = (V + W - 1) // W
    return [(min(r * per, V), max(0, min(per, V - r * per))) for r in range(W)]


def clamp(answers, V):
    return np.clip(np.asarray(answers, np.int64), 0, V - 1)


def range_stats(h, E_rows, answers, base, V):
    """stats [3, Bg] of the rows [base, base + Vs) of a catalogue of V rows: max, sum exp(s - max), s(b, a_b) if owned else 0."""
    h, E_rows = np.asarray(h, np.float64), np.asarray(E_rows, np.float64)
    Bg, Vs = h.shape[0], E_rows.shape[0]
    out = np.zeros((3, Bg))
    out[0] = -np.inf
    if Vs == 0:
        return out
    s = h @ E_rows.T
    out[0] = s.max(axis=1)
    out[1] = np.exp(s - out[0][:, None]).sum(axis=1)
    a = clamp(answers, V) - base
    own = (a >= 0) & (a < Vs)
    out[2, own] = s[np.arange(Bg)[own], a[own]]
    return out


def merge(stats_all):
    """stats_all [W, 3, Bg] in rank order -> (m [Bg], log l [Bg], loss rows [Bg], loss)."""
    stats_all = np.asarray(stats_all, np.float64)
    m, l = np.full(stats_all.shape[2], -np.inf), np.zeros(stats_all.shape[2])
    for m2, l2, _ in stats_all:
        M = np.maximum(m, m2)
        with np.errstate(invalid="ignore"):
            l = np.where(M == -np.inf, l, l * np.exp(m - M) + l2 * np.exp(m2 - M))
        m = M
    logl = np.log(l)
    rows = (m - stats_all[:, 2].sum(axis=0)) + logl
    return m, logl, rows, rows.mean()


def range_bwd(h, E_rows, answers, base, V, m, logl, g=1.0):
    """(dh_part [Bg, d], dE_rows [Vs, d]) of one range from the merged row statistics."""
    h, E_rows = np.asarray(h, np.float64), np.asarray(E_rows, np.float64)
    Bg, Vs = h.shape[0], E_rows.shape[0]
    if Vs == 0:
        return np.zeros_like(h), np.zeros((0, h.shape[1]))
    G = np.exp((h @ E_rows.T - m[:, None]) - logl[:, None])
    a = clamp(answers, V) - base
    own = (a >= 0) & (a < Vs)
    G[np.arange(Bg)[own], a[own]] -= 1.0
    G *= g / Bg
    return G @ E_rows, G.T @ h


def sharded_ce_head(h, E, answers, W, g=1.0):
    """The W ranges of E through stats -> merge -> bwd: (loss, rows, [dh_part per rank], [dE_rows per rank], stats_all)."""
    V = np.asarray(E).shape[0]
    cut = ranges(V, W)
    stats_all = np.stack([range_stats(h, E[lo:lo + vs], answers, lo, V) for lo, vs in cut])
    m, logl, rows, loss = merge(stats_all)
    parts = [range_bwd(h, E[lo:lo + vs], answers, lo, V, m, logl, g) for lo, vs in cut]
    return loss, rows, [p[0] for p in parts], [p[1] for p in parts], stats_all
