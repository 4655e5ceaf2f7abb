"""Evaluation ranking on the host, shared by ``Trainer`` and ``ShardedCatalogue``: the HIP ranking calls behind plain tensors
(operand preparation, workspace, ctypes call and CSR upload are in here), sampled evaluation's host checks, HR / NDCG."""
import numpy as np
import torch

from . import _lib as L

EVAL_FULL_RANK = ("dense", "fused", "rank")
REFERENCE_KS = (5, 10, 20)                      # the reference's cutoffs: the first six returned values
_seen_cache: dict = {}                          # seen_csr: the one uploaded matrix


def eval_full_rank_of(args, full_rank=None) -> str:
    """The evaluation path of ``topk``: ``full_rank`` when given, else ``args.eval_full_rank``, else "dense"."""
    mode = getattr(args, "eval_full_rank", "dense") if full_rank is None else full_rank
    if mode not in EVAL_FULL_RANK:
        raise ValueError(f"eval_full_rank = {mode!r}, expected one of {EVAL_FULL_RANK}")
    return mode


def extra_cutoffs(args) -> tuple:
    """Evaluation cutoffs beyond the reference's 5 / 10 / 20 (``--extra_ks``; none by default)."""
    return tuple(getattr(args, "extra_ks", None) or ())


def sampled_protocol(args):
    """Sampled-candidate evaluation settings (``--eval_negatives / --eval_sampler / --eval_seed``): (negatives per row,
    sampler, seed); 0 negatives = the reference's full-catalogue ranking (the default)."""
    n = int(getattr(args, "eval_negatives", 0) or 0)
    sampler = getattr(args, "eval_sampler", None) or "uniform"
    seed = getattr(args, "eval_seed", None)
    return n, sampler, int(getattr(args, "seed", 0) if seed is None else seed)


def recall_at_k(hit: torch.Tensor, k: int) -> float:
    """src/metrics.py:3-13 for single-target lists: hit is bool[n, K], K >= k."""
    return float(hit[:, :k].any(1).double().mean().item())


def ndcg_at_k(hit: torch.Tensor, k: int) -> float:
    """src/metrics.py:15-31: one relevant item -> idcg = 1, dcg = 1/log2(rank + 2)."""
    w = 1.0 / torch.log2(torch.arange(k, device=hit.device, dtype=torch.float64) + 2.0)
    return float((hit[:, :k].double() * w).sum(1).mean().item())


def sampled_metrics(ranks, k: int):
    """HR@k and NDCG@k of sampled evaluation from the answers' ranks among their candidates (0 = first)."""
    r = np.asarray(ranks, dtype=np.int64)
    hit = r < k
    return float(hit.mean()), float(np.where(hit, 1.0 / np.log2(r.astype(np.float64) + 2.0), 0.0).mean())


def cutoff_metrics(ks, hit=None, ranks=None) -> list:
    """[HR@k, NDCG@k for k in ks] of a hit matrix (bool[n, K], full ranking) or of the answers' ranks (sampled evaluation)."""
    at = (lambda k: sampled_metrics(ranks, k)) if hit is None else (lambda k: (recall_at_k(hit, k), ndcg_at_k(hit, k)))
    return [v for k in ks for v in at(k)]


def metrics_post_fix(epoch, ks, values, protocol=None) -> dict:
    """The log line of ``values = cutoff_metrics(ks, ...)``: "Epoch", HR@k, NDCG@k per cutoff, "Protocol" (sampled only)."""
    post_fix = {"Epoch": epoch}
    for j, k in enumerate(ks):
        post_fix[f"HR@{k}"], post_fix[f"NDCG@{k}"] = '{:.4f}'.format(values[2 * j]), '{:.4f}'.format(values[2 * j + 1])
    if protocol is not None:
        post_fix["Protocol"] = protocol
    return post_fix


def rank_operand(t: torch.Tensor) -> torch.Tensor:
    """``t`` [rows, d] as the ranking kernels read it -- fp32, unit inner stride, 16-byte-aligned base, row stride a multiple of
    4 floats: ``t`` itself when it already is, else a copy of the same values."""
    if t.dtype == torch.float32 and t.stride(1) == 1 and t.data_ptr() % 16 == 0 and t.stride(0) % 4 == 0:
        return t
    c = t.float().contiguous()
    return c.clone() if c.data_ptr() == t.data_ptr() else c          # (fp32 and contiguous, but misaligned: no copy yet)


def seen_csr(matrix, device):
    """The seen-item matrix (scipy CSR, as the reference builds it in src/dataset.py:126-168) on the device as int64
    (indptr, indices) -- uploaded once per matrix."""
    key = (id(matrix), str(device))
    if key not in _seen_cache:
        csr = matrix.tocsr()
        csr.sum_duplicates()
        _seen_cache.clear()
        _seen_cache[key] = (matrix, torch.as_tensor(csr.indptr.astype(np.int64), device=device),
                            torch.as_tensor(csr.indices.astype(np.int64), device=device))
    return _seen_cache[key][1:]


def _ptr(t):
    return None if t is None else t.data_ptr()


def topk_seen(scores, k: int, users=None, csr=None, values: bool = False):
    """``bsarec_topk_seen``: the k best columns of every row of ``scores`` (fp32, unit inner stride), best first, equal scores to
    the smaller column; the seen items of ``users`` in ``csr`` = (indptr, indices) are first set to 0 IN ``scores``."""
    rows, V = scores.shape
    idx = torch.empty(rows, k, dtype=torch.int64, device=scores.device)
    val = torch.empty(rows, k, dtype=torch.float32, device=scores.device) if values else None
    L.check(L.load().bsarec_topk_seen(scores.data_ptr(), scores.stride(0), rows, V, _ptr(users), *map(_ptr, csr or (None, None)),
                                      k, idx.data_ptr(), _ptr(val), torch.cuda.current_stream(scores.device).cuda_stream),
            "bsarec_topk_seen")
    return (idx, val) if values else idx


class FullRank:
    """``bsarec_topk_full_range`` with its workspace: ONE cached buffer, replaced when the call's (B, V, d, k) changes --
    nothing of size O(B V) is ever held.  ``unsupported``: the ValueError text of a shape the kernels do not take.
    A call ranks the rows of ``E`` [V, d] -- rows [base, base + V) of the catalogue -- for every row of ``h`` [B, d] as
    ``topk_seen`` ranks the score matrix; the ids of ``csr`` and the returned ids int64[B, k] are global; ``values``: also the
    fp32 scores (0 for seen items)."""

    def __init__(self, unsupported: str):
        self._unsupported, self._cache = unsupported, (None, None)

    def __call__(self, h, E, k: int, users=None, csr=None, base: int = 0, values: bool = False):
        h, E = rank_operand(h), rank_operand(E.contiguous())
        (B, d), V = h.shape, E.shape[0]
        if self._cache[0] != (B, V, d, k):
            nbytes = L.load().bsarec_topk_full_workspace_bytes(B, V, d, k, 0)
            if nbytes < 0:
                raise ValueError(self._unsupported.format(B=B, V=V, d=d, k=k))
            self._cache = ((B, V, d, k), torch.empty(nbytes, dtype=torch.uint8, device=h.device))
        ws = self._cache[1]
        idx = torch.empty(B, k, dtype=torch.int64, device=h.device)
        val = torch.empty(B, k, dtype=torch.float32, device=h.device) if values else None
        L.check(L.load().bsarec_topk_full_range(h.data_ptr(), h.stride(0), E.data_ptr(), B, V, base, d, _ptr(users),
                                                *map(_ptr, csr or (None, None)), k, 0, ws.data_ptr(), ws.numel(), idx.data_ptr(),
                                                _ptr(val), torch.cuda.current_stream(h.device).cuda_stream), "bsarec_topk_full_range")
        return (idx, val) if values else idx


def _answer_operands(h, E, answers, users, csr):
    h, E = rank_operand(h), rank_operand(E.contiguous())
    ans = answers.to(device=h.device, dtype=torch.int64).contiguous()
    if ans.shape != (h.shape[0],):
        raise ValueError(f"answer_rank: {tuple(ans.shape)} answers for {h.shape[0]} rows")
    return h, E, ans, (_ptr(users), *map(_ptr, csr or (None, None)))


def answer_rank(h, E, answers, users=None, csr=None, base: int = 0, answer_score=None, scores: bool = False):
    """``bsarec_answer_rank_range``: for every row of ``h`` [B, d] the number of items of ``E`` [V, d] -- rows [base, base + V)
    of the catalogue -- that stand before its answer in ``topk_seen``'s order: over the whole catalogue, the answer's index in
    the k = V list, at any depth and without a list.  ``answers`` and the ids of ``csr`` are global; ``answer_score`` (fp32 [B])
    is taken as the answer's score when given (the answer may then belong to another range).  int32 ranks [B] (-1: no valid
    answer); ``scores``: + the answers' fp32 scores (0 for a seen answer, NaN with rank -1)."""
    h, E, ans, seen = _answer_operands(h, E, answers, users, csr)
    (B, d), V = h.shape, E.shape[0]
    if answer_score is not None:
        answer_score = answer_score.to(device=h.device, dtype=torch.float32).contiguous()
    rank = torch.empty(B, dtype=torch.int32, device=h.device)
    val = torch.empty(B, dtype=torch.float32, device=h.device)      # (always: the count launch reads its target there)
    L.check(L.load().bsarec_answer_rank_range(h.data_ptr(), h.stride(0), E.data_ptr(), B, V, base, d, *seen, ans.data_ptr(),
                                              _ptr(answer_score), rank.data_ptr(), val.data_ptr(),
                                              torch.cuda.current_stream(h.device).cuda_stream), "bsarec_answer_rank_range")
    return (rank, val) if scores else rank


def answer_score(h, E, answers, users=None, csr=None, base: int = 0, out=None):
    """``bsarec_answer_score_range``: ``out[b]`` (fp32 [B]; default: zeros) = the effective score of ``answers[b]`` for the rows
    whose answer lies in [base, base + V); the other rows keep their value.  Summed over a catalogue's ranges: the score."""
    h, E, ans, seen = _answer_operands(h, E, answers, users, csr)
    (B, d), V = h.shape, E.shape[0]
    if out is None:
        out = torch.zeros(B, dtype=torch.float32, device=h.device)
    L.check(L.load().bsarec_answer_score_range(h.data_ptr(), h.stride(0), E.data_ptr(), B, V, base, d, *seen, ans.data_ptr(),
                                               out.data_ptr(), torch.cuda.current_stream(h.device).cuda_stream),
            "bsarec_answer_score_range")
    return out


def mrr(ranks) -> float:
    """Mean reciprocal rank of the answers' ranks (0 = first)."""
    r = np.asarray(ranks, dtype=np.float64)
    return float((1.0 / (r + 1.0)).mean())


def sampled_rank(h, E, users, answers, csr, n: int, seed: int, tag: int, cum=None, candidates: bool = False):
    """``bsarec_sampled_rank``: every answer against ``n`` negatives its user has not seen, drawn from the Philox stream of
    (user, tag, seed), uniformly or by ``cum``.  int32 ranks [B] (-1: too few eligible items); ``candidates``: + ids, scores."""
    h, E = rank_operand(h), rank_operand(E.contiguous())
    (B, d), V = h.shape, E.shape[0]
    rank = torch.empty(B, dtype=torch.int32, device=h.device)
    cand = torch.empty(B, n + 1, dtype=torch.int64, device=h.device) if candidates else None
    score = torch.empty(B, n + 1, dtype=torch.float32, device=h.device) if candidates else None
    L.check(L.load().bsarec_sampled_rank(h.data_ptr(), h.stride(0), E.data_ptr(), B, V, d, users.data_ptr(), answers.data_ptr(),
                                         csr[0].data_ptr(), csr[1].data_ptr(), _ptr(cum), n, seed & 0xFFFFFFFFFFFFFFFF, int(tag),
                                         rank.data_ptr(), _ptr(cand), _ptr(score), torch.cuda.current_stream(h.device).cuda_stream),
            "bsarec_sampled_rank")
    return (rank, cand, score) if candidates else rank


def sampling_tables(matrix, sampler: str, popularity, V: int, device):
    """Host tables of the eligibility check and the device cumulative popularity: keys = u * V + item over the seen CSR
    (sorted), seen_w[u] = the drawable items in row u, pool = all drawable items."""
    if sampler == "uniform":
        w = np.ones(V, dtype=np.int64)
    elif sampler == "popularity":
        if popularity is None:
            raise ValueError("sampled_ranks: the popularity sampler needs args.item_popularity (data.item_popularity)")
        pop = np.asarray(popularity, dtype=np.int64)
        if pop.shape != (V,) or pop.min() < 0:
            raise ValueError(f"sampled_ranks: item_popularity must be {V} counts >= 0")
        w = (pop > 0).astype(np.int64)
    else:
        raise ValueError(f"sampled_ranks: unknown sampler {sampler!r}")
    w[0] = 0
    csr = matrix.tocsr()
    csr.sum_duplicates()
    ip, ix = csr.indptr.astype(np.int64), csr.indices.astype(np.int64)
    rows = np.repeat(np.arange(len(ip) - 1, dtype=np.int64), np.diff(ip))
    inr = (ix >= 0) & (ix < V)
    seen_w = np.bincount(rows[inr], weights=w[ix[inr]], minlength=len(ip) - 1).astype(np.int64)
    cum = None if sampler != "popularity" else torch.as_tensor(
        np.cumsum(np.where(np.arange(V) == 0, 0, pop)).astype(np.int64), device=device)
    return {"keys": rows * V + ix, "seen_w": seen_w, "w": w, "pool": int(w.sum()), "cum": cum}


def check_pool(t, users, answers, n: int, V: int):
    """Every row must have >= n drawable items that are neither seen nor its answer (the kernel's -1 is only a backstop)."""
    if ((answers < 1) | (answers >= V)).any():
        i = int(np.nonzero((answers < 1) | (answers >= V))[0][0])
        raise ValueError(f"sampled_ranks: answer {int(answers[i])} of user {int(users[i])} outside [1, {V})")
    q = users * V + answers
    pos = np.minimum(np.searchsorted(t["keys"], q), max(len(t["keys"]) - 1, 0))
    a_seen = (t["keys"][pos] == q) if len(t["keys"]) else np.zeros(len(q), dtype=bool)
    elig = t["pool"] - t["seen_w"][users] - np.where(a_seen, 0, t["w"][answers])
    short = np.nonzero(elig < n)[0]
    if short.size:
        raise ValueError(f"sampled_ranks: {n} negatives requested, but users {users[short[:5]].tolist()} have only "
                         f"{elig[short[:5]].tolist()} eligible items")
