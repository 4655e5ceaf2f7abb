"""Numpy restatement of the full-catalogue ranking order (bsarec_topk_seen / bsarec_topk_full): the seen items of each row
score 0 (not -inf), then a stable descending sort with every NaN equal and above +inf, and -0 equal to +0 -- ties go to the
smaller column."""
import numpy as np


def masked(scores: np.ndarray, seen) -> np.ndarray:
    """scores [B, V] with seen[b] (a list of item ids; ids outside [0, V) ignored) set to +0.0."""
    out = np.array(scores, dtype=np.float32, copy=True)
    V = out.shape[1]
    for b, items in enumerate(seen):
        items = [i for i in items if 0 <= i < V]
        out[b, items] = 0.0
    return out


def order_keys(row: np.ndarray) -> np.ndarray:
    """float64 sort keys whose ascending order is the ranking order: NaN -> -inf-1 (first), -0 -> 0."""
    r = row.astype(np.float64)
    key = -r
    key[np.isnan(r)] = -np.inf
    key[key == 0] = 0.0
    return key


def topk(scores: np.ndarray, seen, k: int):
    """(ids [B, k] int64, values [B, k] float32) of the masked rows under the total order."""
    m = masked(scores, seen)
    ids = np.empty((m.shape[0], k), np.int64)
    for b in range(m.shape[0]):
        key = order_keys(m[b])
        nan = np.isnan(m[b])
        # NaN first (smaller column first), then the stable sort of the rest
        idx = np.concatenate([np.nonzero(nan)[0], np.nonzero(~nan)[0][np.argsort(key[~nan], kind="stable")]])
        ids[b] = idx[:k]
    return ids, np.take_along_axis(m, ids, axis=1)
