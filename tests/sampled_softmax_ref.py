"""Numpy restatement of the sampled-softmax training head (``bsarec_config_t.train_negatives``, include/bsarec_hip.h): the
draw stream, the logQ corrections, the logits with the accidental-hit mask, the loss and its gradients -- written from the
header's contract and nothing else.  Built on the oracle's Philox; ``oracle_head`` plugs it into ``loss_and_grads(head=)``."""
import numpy as np

from oracle.bsarec_oracle import philox4x32_10
from sampled_eval_ref import mulhi64

TRAIN_NEG_MAX = 8192
SITE = 0x4E454753
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def cumulative(counts) -> np.ndarray:
    """The header's table: int64[V], cum[0] = 0 (item 0 is never drawn), cum[i] = counts[1] + ... + counts[i]."""
    c = np.asarray(counts, dtype=np.int64)
    return np.cumsum(np.where(np.arange(c.shape[0]) == 0, 0, c))


def draws(seed: int, step: int, V: int, N: int, cum=None) -> np.ndarray:
    """The N candidates of a step: Philox call j has counter (lo32 j, hi32 j, SITE, lo32 step), key (lo32 seed, hi32 seed).
    Uniform: 4 draws per call, 1 + (w (V - 1) >> 32); popularity: 2 per call, the smallest i with cum[i] > mulhi64(x, T)."""
    per = 4 if cum is None else 2
    j = np.arange(-(-N // per), dtype=np.uint64)
    w = philox4x32_10(j & _M32, j >> _S32, SITE, step & 0xFFFFFFFF, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    w = [np.asarray(x, dtype=np.uint64) for x in w]
    if cum is None:
        words = np.stack(w, axis=1).reshape(-1)[:N]
        return (1 + ((words * np.uint64(V - 1)) >> _S32)).astype(np.int64)
    cum = np.asarray(cum, dtype=np.int64)
    x = np.stack([w[0] | (w[1] << _S32), w[2] | (w[3] << _S32)], axis=1).reshape(-1)[:N]
    r = mulhi64(x, int(cum[-1]))
    return np.searchsorted(cum, r.astype(np.int64), side="right").astype(np.int64)


def corrections(items, N: int, cum=None, logq: bool = True) -> np.ndarray:
    """c(i) = log(N q_i), q_i = count_i / T (popularity sampler, logQ on); 0 otherwise.  float64."""
    items = np.asarray(items, dtype=np.int64)
    if cum is None or not logq:
        return np.zeros(items.shape, dtype=np.float64)
    cum = np.asarray(cum, dtype=np.int64)
    prev = np.where(items > 0, cum[np.maximum(items - 1, 0)], 0)
    return np.log(N * (cum[items] - prev).astype(np.float64) / float(cum[-1]))


def head(h, E, answers, cand, cum=None, logq: bool = True):
    """float64 head on the given h [B, d], E [V, d]: (x [B, N + 1], loss_rows [B], loss, g = dloss/dx [B, N + 1])."""
    h, E = np.asarray(h, dtype=np.float64), np.asarray(E, dtype=np.float64)
    answers, cand = np.asarray(answers, dtype=np.int64), np.asarray(cand, dtype=np.int64)
    N, B = cand.shape[0], h.shape[0]
    cols = np.concatenate([answers[:, None], np.broadcast_to(cand[None, :], (B, N))], axis=1)       # [B, N + 1]
    x = np.einsum("bd,bcd->bc", h, E[cols]) - corrections(cols, N, cum, logq)
    x[:, 1:][cand[None, :] == answers[:, None]] = -np.inf                                            # accidental hits
    mx = x.max(axis=1, keepdims=True)
    lse = mx[:, 0] + np.log(np.exp(x - mx).sum(axis=1))
    loss_rows = lse - x[:, 0]
    g = np.exp(x - lse[:, None])
    g[:, 0] -= 1.0
    g /= B
    return x, loss_rows, float(loss_rows.mean()), g


def grads(h, E, answers, cand, cum=None, logq: bool = True):
    """(loss, dh [B, d], dE [V, d]) in float64: dh_b = sum_c g_bc E[c], dE[c] += g_bc h_b over every column."""
    h64, E64 = np.asarray(h, dtype=np.float64), np.asarray(E, dtype=np.float64)
    B, N = h64.shape[0], len(cand)
    _, _, loss, g = head(h64, E64, answers, cand, cum, logq)
    cols = np.concatenate([np.asarray(answers, dtype=np.int64)[:, None], np.broadcast_to(np.asarray(cand)[None, :], (B, N))], axis=1)
    dh = np.einsum("bc,bcd->bd", g, E64[cols])
    dE = np.zeros_like(E64)
    np.add.at(dE, cols.reshape(-1), (g[:, :, None] * h64[:, None, :]).reshape(-1, h64.shape[1]))
    return loss, dh, dE


def oracle_head(answers, cand, cum=None, logq: bool = True):
    """``head`` argument of oracle.bsarec_oracle.loss_and_grads: this sampled softmax on the oracle's h_last."""
    def fn(h_last, E, dtype):
        loss, dh, dE = grads(h_last, E, answers, cand, cum, logq)
        return loss, None, dE.astype(dtype), dh.astype(dtype)
    return fn
