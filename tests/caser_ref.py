"""fp64 numpy restatement of the Caser convolution block of bsarec_caser_fwd / bsarec_caser_bwd (include/bsarec_hip.h): the vertical
filters, one horizontal filter bank per height h = 1 .. L with ReLU and the maximum over positions, every gradient, the padded flat
weight layout, and the model's head (Linear + ReLU on the dropped-out features, GRU4Rec's pairwise BPR).  Checked against
torch.nn.Conv2d / F.max_pool1d / nn.Linear in double by tests/test_caser_cpu.py; the GPU tests compare the kernels with it.

Tie rule: a cell's maximum is attained at every t with max - c[t] <= TIE (1e-12, far below fp64 noise of O(1) sums of these sizes
and far above nothing: exact ties come from bit-identical windows); the LOWEST such t takes the gradient, and only if max > 0."""
import numpy as np

TIE = 1e-12


def weight_shapes(L, d, nh, nv):
    """(name, shape) of the flat weight array, in its order."""
    out = [("conv_v.weight", (nv, L)), ("conv_v.bias", (nv,))]
    for h in range(1, L + 1):
        out += [(f"conv_h.{h - 1}.weight", (nh, h, d)), (f"conv_h.{h - 1}.bias", (nh,))]
    return out


def layout(L, d, nh, nv):
    """([(name, offset, shape)], total floats): every tensor starts at a multiple of 4 floats."""
    out, off = [], 0
    for name, shp in weight_shapes(L, d, nh, nv):
        off = (off + 3) // 4 * 4
        out.append((name, off, shp))
        off += int(np.prod(shp))
    return out, (off + 3) // 4 * 4


def weight_floats(L, d, nh, nv):
    return layout(L, d, nh, nv)[1]


def split_weights(flat, L, d, nh, nv):
    """The flat array -> {name: array} (views)."""
    lay, total = layout(L, d, nh, nv)
    assert flat.size == total
    return {name: flat[off:off + int(np.prod(shp))].reshape(shp) for name, off, shp in lay}


def flat_weights(w, L, d, nh, nv, dtype=np.float64):
    """{name: array} -> the flat array, zeros in the gaps."""
    lay, total = layout(L, d, nh, nv)
    flat = np.zeros(total, dtype)
    for name, off, shp in lay:
        flat[off:off + int(np.prod(shp))] = np.asarray(w[name]).reshape(-1)
    return flat


def random_case(shape):
    """(x [B, L, d] fp32, flat weights fp32) of a shape (B, L, d, n_h, n_v): x ~ N(0, 1), every filter and bias U(+-1/sqrt(fan_in))."""
    B, L, d, nh, nv = shape
    rng = np.random.default_rng(sum(p * v for p, v in zip((7, 11, 13, 17, 19), shape)))
    x = rng.normal(0, 1, (B, L, d)).astype(np.float32)
    w = {}
    bv = 1.0 / np.sqrt(L)
    w["conv_v.weight"] = rng.uniform(-bv, bv, (nv, L))
    w["conv_v.bias"] = rng.uniform(-bv, bv, nv)
    for h in range(1, L + 1):
        bh = 1.0 / np.sqrt(h * d)
        w[f"conv_h.{h - 1}.weight"] = rng.uniform(-bh, bh, (nh, h, d))
        w[f"conv_h.{h - 1}.bias"] = rng.uniform(-bh, bh, nh)
    return x, flat_weights(w, L, d, nh, nv, np.float32)


def windows(x, h):
    """[B, L - h + 1, h d]: window t is rows t .. t + h - 1 of a sequence, flattened."""
    B, L, d = x.shape
    return np.stack([x[:, t:t + h].reshape(B, h * d) for t in range(L - h + 1)], 1)


def forward(x, flat, nh, nv):
    """x [B, L, d], flat weights -> (z [B, n_v d + n_h L], cache for backward / ambiguous)."""
    x = np.asarray(x, np.float64)
    B, L, d = x.shape
    w = split_weights(np.asarray(flat, np.float64), L, d, nh, nv)
    zv = np.einsum("ct,btj->bcj", w["conv_v.weight"], x) + w["conv_v.bias"][None, :, None]
    zh = np.zeros((B, L, nh))
    tstar = np.zeros((B, L, nh), np.int64)
    passes = np.zeros((B, L, nh), bool)
    cs = []
    for h in range(1, L + 1):
        c = np.einsum("btk,fk->bft", windows(x, h), w[f"conv_h.{h - 1}.weight"].reshape(nh, h * d))
        c = c + w[f"conv_h.{h - 1}.bias"][None, :, None]
        m = c.max(-1)
        tstar[:, h - 1] = np.argmax(m[..., None] - c <= TIE, -1)          # the first (lowest) tied t
        passes[:, h - 1] = m > 0
        zh[:, h - 1] = np.maximum(m, 0.0)
        cs.append(c)
    z = np.concatenate([zv.reshape(B, nv * d), zh.reshape(B, L * nh)], 1)
    return z, (x, w, tstar, passes, cs, (B, L, d, nh, nv))


def backward(cache, dz):
    """dz [B, F] -> (dx [B, L, d], dflat in the padded layout, zeros in the gaps)."""
    x, w, tstar, passes, cs, (B, L, d, nh, nv) = cache
    dz = np.asarray(dz, np.float64)
    dzv = dz[:, :nv * d].reshape(B, nv, d)
    g = dz[:, nv * d:].reshape(B, L, nh) * passes
    grads = {"conv_v.weight": np.einsum("bcj,btj->ct", dzv, x), "conv_v.bias": dzv.sum((0, 2))}
    dx = np.einsum("ct,bcj->btj", w["conv_v.weight"], dzv)
    for h in range(1, L + 1):
        Wh = w[f"conv_h.{h - 1}.weight"]
        gh, th = g[:, h - 1], tstar[:, h - 1]                             # [B, n_h]
        xw = windows(x, h)                                                # [B, T, h d]
        win = xw[np.arange(B)[:, None], th]                               # [B, n_h, h d]
        grads[f"conv_h.{h - 1}.weight"] = np.einsum("bf,bfk->fk", gh, win).reshape(nh, h, d)
        grads[f"conv_h.{h - 1}.bias"] = gh.sum(0)
        for b in range(B):
            for f in range(nh):
                if gh[b, f] != 0.0:
                    dx[b, th[b, f]:th[b, f] + h] += gh[b, f] * Wh[f]
    return dx, flat_weights(grads, L, d, nh, nv)


def ambiguous(cache, margin):
    """bool [B, L, n_h]: cells whose discrete choice fp32 cannot be asked to reproduce -- |max| < margin (ReLU's switch), or some t
    that is not tied with the maximum and yet within margin of it (the argmax)."""
    cs = cache[4]
    out = []
    for c in cs:
        m = c.max(-1)
        gap = m[..., None] - c
        out.append((np.abs(m) < margin) | ((gap > TIE) & (gap < margin)).any(-1))
    return np.stack(out, 1)


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def bpr(s, pos, neg):
    """loss = mean_b -log(sigmoid(s . pos - s . neg) + 1e-10); returns (loss, ds, dpos, dneg)."""
    s, pos, neg = (np.asarray(v, np.float64) for v in (s, pos, neg))
    diff = (s * pos).sum(-1) - (s * neg).sum(-1)
    sg = sigmoid(diff)
    loss = float(np.mean(-np.log(sg + 1e-10)))
    dd = (-(sg * (1 - sg)) / (sg + 1e-10) / s.shape[0])[:, None]
    return loss, dd * (pos - neg), dd * s, -dd * s


def model_loss_grads(E, flat, fc_w, fc_b, ids, pos_ids, neg_ids, nh, nv, keep=None, p=0.0):
    """The whole model in double: x = E[ids], z = conv(x), s = relu(fc1(z * keep / (1 - p))), BPR.  Returns (loss, s,
    {state_dict key: gradient}) with the conv gradients as one flat array under "conv"."""
    E, fc_w, fc_b = (np.asarray(v, np.float64) for v in (E, fc_w, fc_b))
    z, cache = forward(E[ids], flat, nh, nv)
    scale = np.ones_like(z) if keep is None else np.asarray(keep, np.float64) / (1.0 - p)
    zd = z * scale
    pre = zd @ fc_w.T + fc_b
    s = np.maximum(pre, 0.0)
    loss, ds, dpos, dneg = bpr(s, E[pos_ids], E[neg_ids])
    dpre = ds * (pre > 0)
    dzd = dpre @ fc_w
    dx, dflat = backward(cache, dzd * scale)
    dE = np.zeros_like(E)
    np.add.at(dE, ids.reshape(-1), dx.reshape(-1, E.shape[1]))
    np.add.at(dE, pos_ids, dpos)
    np.add.at(dE, neg_ids, dneg)
    return loss, s, {"item_embeddings.weight": dE, "conv": dflat, "fc1.weight": dpre.T @ zd, "fc1.bias": dpre.sum(0)}
