"""fp64 numpy restatement of BERT4Rec's cloze step (include/bsarec_hip.h: bsarec_cloze_mask, bsarec_cloze_head_fwd / _bwd, and the
plan option bidirectional): the masking rule on the oracle's Philox stream, the head on a row list, and the oracle's encoder
under the padding-only attention mask."""
import contextlib

import numpy as np

from oracle import bsarec_oracle as O

CLOZE_SITE = 0x434C4F5A


def ratio_f32(ratio):
    """The ratio as the C ABI sees it (a float argument)."""
    return float(np.float32(ratio))


def cloze_mask(ids, ratio, slots, seed, step, mask_token):
    """ids int64 [B, L] -> (masked_ids [B, L], rows int32 [B slots], targets int64 [B slots], n).  Token e = b L + t is drawn when
    ids > 0 and its word of the stream of dropout_keep(B L, ratio, seed, step, CLOZE_SITE) is BELOW the threshold (i.e. the
    dropout mask would drop it); a row that draws nothing and ends in an item draws its last position; the loss positions of a
    row are its last min(count, slots) drawn ones; rows: their token indices ascending, -1 / 0 behind the n live ones."""
    ids = np.asarray(ids, np.int64)
    B, L = ids.shape
    keep = O.dropout_keep(B * L, ratio_f32(ratio), int(seed), int(step), CLOZE_SITE).reshape(B, L)
    drawn = (ids > 0) & ~keep
    for b in range(B):
        if not drawn[b].any() and ids[b, L - 1] > 0:
            drawn[b, L - 1] = True
    masked = np.where(drawn, np.int64(mask_token), ids)
    R = B * slots
    rows, targets = np.full(R, -1, np.int32), np.zeros(R, np.int64)
    n = 0
    for b in range(B):
        pos = np.nonzero(drawn[b])[0][-slots:]
        for t in pos:
            rows[n], targets[n] = b * L + t, ids[b, t]
            n += 1
    return masked, rows, targets, n


def cloze_head(h, E, rows, targets, n, g=1.0):
    """h [T, d], E [V, d] (the classes), rows / targets as cloze_mask writes them, n live rows, upstream scalar g ->
    (loss, row losses [R], dh [T, d], dE [V, d])."""
    h, E = np.asarray(h, np.float64), np.asarray(E, np.float64)
    R, V = len(rows), E.shape[0]
    n = max(0, min(int(n), R))
    out_rows, dh, dE = np.zeros(R), np.zeros_like(h), np.zeros_like(E)
    if n == 0:
        return 0.0, out_rows, dh, dE
    idx = np.asarray(rows[:n], np.int64)
    a = np.clip(np.asarray(targets[:n], np.int64), 0, V - 1)
    s = h[idx] @ E.T
    m = s.max(axis=1, keepdims=True)
    lse = m[:, 0] + np.log(np.exp(s - m).sum(axis=1))
    out_rows[:n] = lse - s[np.arange(n), a]
    G = np.exp(s - lse[:, None])
    G[np.arange(n), a] -= 1.0
    G *= g / n
    dh[idx] = G @ E                                  # the rows are distinct
    dE[:] = G.T @ h[idx]
    return out_rows[:n].sum() / n, out_rows, dh, dE


def padding_mask(ids):
    """Additive padding-only mask in {0, -10000}, [B, 1, L, L]: the oracle's attention_mask without its causal term."""
    B, L = ids.shape
    key_ok = np.broadcast_to((ids > 0)[:, None, None, :], (B, 1, L, L))
    return (1.0 - key_ok.astype(np.float64)) * -10000.0


@contextlib.contextmanager
def bidirectional_oracle():
    """oracle.forward / loss_and_grads under the padding-only mask, restored afterwards."""
    old = O.attention_mask
    O.attention_mask = padding_mask
    try:
        yield O
    finally:
        O.attention_mask = old


def null_head(h_last, E, dtype):
    """A loss head that contributes nothing: loss_and_grads(d_outs=..., head=null_head) backpropagates d_outs alone."""
    return 0.0, None, np.zeros_like(E), np.zeros_like(h_last)
