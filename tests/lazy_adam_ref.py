"""Numpy restatement of lazy (sparse) Adam for the item table (``bsarec_config_t.train_lazy_adam``, include/bsarec_hip.h),
written from the header's contract: the touched set of a step and the float32 update of its rows, in the kernel's
operation order, with the bias corrections of the step tick (running products in float64).  The dense update shares the
arithmetic (``dense_step``); ``dense_grad`` forms its gradient from the sources of ``bsarec_adam_t`` as ``adam_kernel`` does, and
``adam_f64`` is a float64 Adam with ``pow`` as an independent second opinion (tests/test_gpu_dense_adam.py)."""
import numpy as np


def touched(ids, answers, cand, V: int) -> np.ndarray:
    """T = {ids != 0} u {answers} u {candidates}, ids and answers clamped to [0, V) as the kernels read them; sorted."""
    ids = np.clip(np.asarray(ids, dtype=np.int64).reshape(-1), 0, V - 1)
    ans = np.clip(np.asarray(answers, dtype=np.int64).reshape(-1), 0, V - 1)
    return np.unique(np.concatenate([ids[ids != 0], ans, np.asarray(cand, dtype=np.int64).reshape(-1)]))


def corrections(t: int, lr: float, b1: float, b2: float):
    """(step_size, bc2s) of Adam step t >= 1: lr / (1 - b1^t) and sqrt(1 - b2^t) from float64 running products of the
    float32 betas, each rounded once to float32."""
    p1 = p2 = 1.0
    for _ in range(t):
        p1 *= float(np.float32(b1))
        p2 *= float(np.float32(b2))
    return np.float32(float(np.float32(lr)) / (1.0 - p1)), np.float32(np.sqrt(1.0 - p2))


def lazy_step(w, m, v, g_rows, rows, t: int, lr: float, b1: float, b2: float, eps: float, wd: float):
    """One lazy step on the item table: ``w``, ``m``, ``v`` float32 [V, d]; ``g_rows`` [|T|, d] the gradient rows of the
    sorted unique ``rows``.  Returns new (w, m, v); rows outside T are copied unchanged."""
    w, m, v = (np.array(x, dtype=np.float32, copy=True) for x in (w, m, v))
    f32 = np.float32
    b1, b2, eps, wd = f32(b1), f32(b2), f32(eps), f32(wd)
    step_size, bc2s = corrections(t, lr, b1, b2)
    r = np.asarray(rows, dtype=np.int64)
    g = np.asarray(g_rows, dtype=np.float32)
    wr, mr, vr = w[r], m[r], v[r]
    if wd != 0:
        g = g + wd * wr
    mr = b1 * mr + (f32(1) - b1) * g
    vr = b2 * vr + (f32(1) - b2) * g * g
    wr = wr - step_size * (mr / (np.sqrt(vr) / bc2s + eps))
    w[r], m[r], v[r] = wr, mr, vr
    return w, m, v


def dense_step(w, m, v, g, t: int, lr: float, b1: float, b2: float, eps: float, wd: float):
    """The dense update of the same table: every row, ``g`` [V, d]."""
    return lazy_step(w, m, v, g, np.arange(np.asarray(w).shape[0]), t, lr, b1, b2, eps, wd)


def dense_grad(grads, w, grad_scale: float = 1.0, wd: float = 0.0, grads2=None, grads2_n: int = 0, srcs=None):
    """The gradient as the dense Adam kernel forms it (``bsarec_adam_t``, include/bsarec_hip.h), in float32 and in the kernel's
    order: the sum of the sources ``srcs`` in index order (``grads`` is then ignored), else ``grads`` plus ``grads2`` on the first
    ``grads2_n`` elements; then times ``grad_scale``; then ``+ wd * w``.  Hand the result to :func:`dense_step` with ``wd = 0``."""
    f32 = np.float32
    if srcs:
        g = np.array(srcs[0], dtype=np.float32, copy=True)
        for s in srcs[1:]:
            g = g + np.asarray(s, dtype=np.float32)
    else:
        g = np.array(grads, dtype=np.float32, copy=True)
        if grads2 is not None:
            g[:grads2_n] = g[:grads2_n] + np.asarray(grads2, dtype=np.float32)[:grads2_n]
    g = g * f32(grad_scale)
    if f32(wd) != 0:
        g = g + f32(wd) * np.asarray(w, dtype=np.float32)
    return g


def adam_f64(w, m, v, g, t: int, lr: float, b1: float, b2: float, eps: float, wd: float = 0.0):
    """torch.optim.Adam's step t >= 1 in float64 with ``pow(beta, t)``: a second opinion that shares neither the operation order
    nor the running products of the restatement above.  The hyper-parameters are the float32 values the C ABI carries (1 - beta2
    of 0.999 differs by 3e-5 relative between float32 and float64)."""
    w, m, v, g = (np.asarray(x, dtype=np.float64) for x in (w, m, v, g))
    lr, b1, b2, eps, wd = (float(np.float32(x)) for x in (lr, b1, b2, eps, wd))
    g = g + wd * w
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    denom = np.sqrt(v) / np.sqrt(1.0 - pow(b2, t)) + eps
    return w - lr / (1.0 - pow(b1, t)) * m / denom, m, v
