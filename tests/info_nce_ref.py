"""DuoRec's contrastive head (bsarec_info_nce_fwd / _bwd, include/bsarec_hip.h) restated in numpy fp64: the closed forms of
the loss and of its gradient, no autograd.  z = [z_i; z_j], n = 2B, pos(r) = (r + B) mod n."""
import numpy as np

EPS = 1e-8                                   # torch.nn.functional.cosine_similarity clamps each norm on its own


def info_nce(z_i, z_j, tau, sim="dot", g=1.0):
    """-> (loss, rows[2B], dz_i[B, d], dz_j[B, d]) in fp64 for the upstream scalar g."""
    z = np.concatenate([np.asarray(z_i, np.float64), np.asarray(z_j, np.float64)], axis=0)
    n, B = z.shape[0], z.shape[0] // 2
    norm = np.sqrt((z * z).sum(1))
    clamped = np.maximum(norm, EPS)
    u = z / clamped[:, None] if sim == "cos" else z
    s = u @ u.T / tau
    off = s.copy()
    np.fill_diagonal(off, -np.inf)
    mx = off.max(1)
    lse = mx + np.log(np.exp(off - mx[:, None]).sum(1))
    pos = (np.arange(n) + B) % n
    rows = lse - s[np.arange(n), pos]
    loss = rows.mean()
    W = np.exp(off - lse[:, None]) + np.exp(off - lse[None, :])          # exp(-inf) = 0 on the diagonal
    du = g / (n * tau) * (W @ u - 2.0 * u[pos])
    if sim == "cos":
        proj = (du - u * (u * du).sum(1, keepdims=True)) / clamped[:, None]
        dz = np.where((norm > EPS)[:, None], proj, du / EPS)
    else:
        dz = du
    return loss, rows, dz[:B], dz[B:]
