"""Numpy restatement of the answer-rank contract (bsarec_answer_rank / _range / bsarec_answer_score_range, include/bsarec_hip.h)
from a RAW score matrix over the whole catalogue and per-row lists of seen GLOBAL ids: the effective score of a seen item is
+0.0; the rank of (t, a) is the number of items j != a of the range whose 32-bit order key is above t's, or equal with j < a."""
import numpy as np

import full_rank_ref as R


def order_key(v) -> np.ndarray:
    """uint32 keys whose unsigned order is the score order: every NaN one value above +inf, -0 = +0."""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).copy()
    u[(u & 0x7fffffff) > 0x7f800000] = 0x7fc00000
    u[u == 0x80000000] = 0
    neg = (u & 0x80000000) != 0
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def answer_scores(scores, seen, answers, lo=0, hi=None, out=None) -> np.ndarray:
    """out[b] = e(b, answers[b]) for the rows whose answer lies in [lo, hi); the other rows keep their value (default 0)."""
    e = R.masked(scores, seen)
    hi = e.shape[1] if hi is None else hi
    out = np.zeros(e.shape[0], np.float32) if out is None else out
    for b, a in enumerate(answers):
        if lo <= a < hi:
            out[b] = e[b, a]
    return out


def ranks(scores, seen, answers, lo=0, hi=None, answer_score=None):
    """(int32 ranks [B], float32 scores [B]) of the range [lo, hi) of the catalogue ``scores`` [B, V] spans."""
    e = R.masked(scores, seen)
    B, V = e.shape
    hi = V if hi is None else hi
    rank, val = np.full(B, -1, np.int32), np.full(B, np.nan, np.float32)
    cols = np.arange(lo, hi)
    for b, a in enumerate(answers):
        a = int(a)
        if answer_score is None:
            if not lo <= a < hi:
                continue
            t = e[b, a]
        else:
            if not 0 <= a < 2 ** 31:
                continue
            t = np.float32(answer_score[b])
        key, tk = order_key(e[b, lo:hi]), order_key(np.array([t], np.float32))[0]
        before = (key > tk) | ((key == tk) & (cols < a))
        rank[b], val[b] = int((before & (cols != a)).sum()), t
    return rank, val


def index_in_full_list(scores, seen, answers) -> np.ndarray:
    """The index of answers[b] in full_rank_ref.topk(scores, seen, k = V): the definition the ranks restate."""
    ids, _ = R.topk(scores, seen, scores.shape[1])
    return np.array([int(np.nonzero(ids[b] == a)[0][0]) for b, a in enumerate(answers)], np.int32)
