"""Numpy restatement of sampled-candidate evaluation (``bsarec_sampled_rank``, include/bsarec_hip.h): the draw stream, the
acceptance rule, the rank and the metrics, written from the protocol and nothing else.  Built on the oracle's Philox."""
import numpy as np

from oracle.bsarec_oracle import philox4x32_10

NEG_MAX = 1024
NEG_MAX_DRAWS = 1 << 20
_M32 = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def mulhi64(x, t: int):
    """High 64 bits of the 128-bit products x * t (x uint64 array, 0 <= t < 2^64), by 32-bit limbs."""
    x = np.asarray(x, dtype=np.uint64)
    xl, xh = x & _M32, x >> _S32
    tl, th = np.uint64(t & 0xFFFFFFFF), np.uint64(t >> 32)
    ll, lh, hl, hh = xl * tl, xl * th, xh * tl, xh * th
    mid = (ll >> _S32) + (lh & _M32) + (hl & _M32)
    return hh + (lh >> _S32) + (hl >> _S32) + (mid >> _S32)


def draw_items(user: int, tag: int, seed: int, V: int, first_call: int, n_calls: int, cum=None) -> np.ndarray:
    """Items of the draws made by Philox calls first_call .. first_call + n_calls - 1, in stream order
    (uniform: 4 per call; popularity, cum given: 2 per call)."""
    j = np.arange(first_call, first_call + n_calls, dtype=np.uint64)
    user &= 0xFFFFFFFFFFFFFFFF
    w = philox4x32_10(j, user & 0xFFFFFFFF, user >> 32, tag, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    w = [np.asarray(x, dtype=np.uint64) for x in w]
    if cum is None:
        words = np.stack(w, axis=1).reshape(-1)                               # draw 4j + m takes w_m
        return (1 + ((words * np.uint64(V - 1)) >> _S32)).astype(np.int64)
    cum = np.asarray(cum, dtype=np.int64)
    x = np.stack([w[0] | (w[1] << _S32), w[2] | (w[3] << _S32)], axis=1).reshape(-1)   # draw 2j + m: w_2m | w_2m+1 << 32
    r = mulhi64(x, int(cum[-1]))
    return np.searchsorted(cum, r.astype(np.int64), side="right").astype(np.int64)   # smallest i with cum[i] > r


def candidates(user: int, answer: int, seen, seed: int, tag: int, V: int, n: int, cum=None):
    """[answer, n_1 .. n_n] of one row, or None when the row fails (fewer than n accepted within NEG_MAX_DRAWS draws)."""
    seen = np.asarray(seen, dtype=np.int64)
    per = 2 if cum is not None else 4
    chunk = 4096                                                              # Philox calls per step (any size gives the same)
    acc = np.zeros(0, dtype=np.int64)
    for c0 in range(0, NEG_MAX_DRAWS // per, chunk):
        items = draw_items(user, tag, seed, V, c0, min(chunk, NEG_MAX_DRAWS // per - c0), cum)
        ok = (items != answer) & ~np.isin(items, seen)
        e = items[ok]
        uniq, first = np.unique(e, return_index=True)
        new = uniq[np.argsort(first)]                                         # first occurrence, stream order
        new = new[~np.isin(new, acc)]
        acc = np.concatenate([acc, new[:n - len(acc)]])
        if len(acc) == n:
            return np.concatenate([[answer], acc]).astype(np.int64)
    return None


def rank_of(scores) -> int:
    """scores[0] = the answer's, scores[1:] the negatives': ties and NaN negatives count against the model; NaN answer -> N."""
    s = np.asarray(scores)
    sa, neg = s[0], s[1:]
    if np.isnan(sa):
        return len(neg)
    return int(np.count_nonzero((neg > sa) | (neg == sa) | np.isnan(neg)))


def metrics(ranks, ks=(5, 10, 20)):
    """[HR@k, NDCG@k for k in ks] from ranks (0 = first)."""
    r = np.asarray(ranks, dtype=np.int64)
    out = []
    for k in ks:
        hit = r < k
        out += [float(hit.mean()), float(np.where(hit, 1.0 / np.log2(r + 2.0), 0.0).mean())]
    return out


def eligible_count(answer: int, seen, V: int, pop=None) -> int:
    """Items the row can draw: in [1, V), count > 0 for the popularity sampler, not seen, not the answer."""
    ok = np.ones(V, dtype=bool) if pop is None else np.asarray(pop) > 0
    ok[0] = False
    s = np.asarray(seen, dtype=np.int64)
    ok[s[(s >= 0) & (s < V)]] = False
    ok[answer] = False
    return int(ok.sum())
