"""fp64 numpy restatement of the GRU stack of bsarec_gru_fwd / bsarec_gru_bwd (include/bsarec_hip.h): N bias-free GRU layers in
torch's gate order (r, z, n) with h_0 = 0, an optional Linear on top, every gradient, and GRU4Rec's BPR head.  Checked against
torch.nn.GRU / nn.Linear in double by tests/test_gru_cpu.py; the GPU tests compare the kernels with it."""
import numpy as np


def sigmoid(x):
    return 1.0 / (1.0 + np.exp(-x))


def weight_shapes(I, H, N, O):
    """(name, shape) of the flat weight array, in its order."""
    out = []
    for k in range(N):
        out += [(f"weight_ih_l{k}", (3 * H, I if k == 0 else H)), (f"weight_hh_l{k}", (3 * H, H))]
    if O:
        out += [("out_weight", (O, H)), ("out_bias", (O,))]
    return out


def split_weights(flat, I, H, N, O):
    """The flat array -> {name: array} (views)."""
    w, off = {}, 0
    for name, shp in weight_shapes(I, H, N, O):
        n = int(np.prod(shp))
        w[name] = flat[off:off + n].reshape(shp)
        off += n
    assert off == flat.size
    return w


def flat_weights(w, I, H, N, O):
    return np.concatenate([np.asarray(w[name]).reshape(-1) for name, _ in weight_shapes(I, H, N, O)])


def random_weights(rng, I, H, N, O, scale=1.0):
    """U(-1/sqrt(H), 1/sqrt(H)) rounded to fp32 (the projection too), as one flat fp32 array."""
    n = sum(int(np.prod(s)) for _, s in weight_shapes(I, H, N, O))
    b = 1.0 / np.sqrt(H)
    return (rng.uniform(-b, b, n) * scale).astype(np.float32)


def forward(x, flat, H, N, O):
    """x [B, L, I], flat weights -> (out [B, L, O or H], cache for backward)."""
    x = np.asarray(x, np.float64)
    B, L, I = x.shape
    w = split_weights(np.asarray(flat, np.float64), I, H, N, O)
    inp, layers = x, []
    for k in range(N):
        wih, whh = w[f"weight_ih_l{k}"], w[f"weight_hh_l{k}"]
        a = inp @ wih.T                                   # [B, L, 3H]
        h = np.zeros((B, H))
        Y = np.zeros((B, L, H))
        R, Z, Nn, Bn = (np.zeros((B, L, H)) for _ in range(4))
        for t in range(L):
            b = h @ whh.T
            r = sigmoid(a[:, t, :H] + b[:, :H])
            z = sigmoid(a[:, t, H:2 * H] + b[:, H:2 * H])
            n = np.tanh(a[:, t, 2 * H:] + r * b[:, 2 * H:])
            h = n + z * (h - n)
            Y[:, t], R[:, t], Z[:, t], Nn[:, t], Bn[:, t] = h, r, z, n, b[:, 2 * H:]
        layers.append((inp, Y, R, Z, Nn, Bn))
        inp = Y
    out = inp @ w["out_weight"].T + w["out_bias"] if O else inp
    return out, (w, layers, (B, L, I, H, N, O))


def backward(cache, dout):
    """dout [B, L, O or H] -> (dx [B, L, I], dflat in the layout of the flat weights)."""
    w, layers, (B, L, I, H, N, O) = cache
    dout = np.asarray(dout, np.float64)
    g = {}
    if O:
        y = layers[-1][1]
        g["out_weight"] = dout.reshape(-1, O).T @ y.reshape(-1, H)
        g["out_bias"] = dout.reshape(-1, O).sum(0)
        dY = dout @ w["out_weight"]
    else:
        dY = dout
    for k in range(N - 1, -1, -1):
        inp, Y, R, Z, Nn, Bn = layers[k]
        wih, whh = w[f"weight_ih_l{k}"], w[f"weight_hh_l{k}"]
        dh = np.zeros((B, H))
        da = np.zeros((B, L, 3 * H))
        dwhh = np.zeros_like(whh)
        for t in range(L - 1, -1, -1):
            hp = Y[:, t - 1] if t > 0 else np.zeros((B, H))
            r, z, n, bn = R[:, t], Z[:, t], Nn[:, t], Bn[:, t]
            gt = dY[:, t] + dh
            dn = gt * (1 - z)
            dz = gt * (hp - n)
            dh = gt * z
            dan = dn * (1 - n * n)
            dbn = dan * r
            dr = dan * bn
            dar = dr * r * (1 - r)
            daz = dz * z * (1 - z)
            db = np.concatenate([dar, daz, dbn], 1)
            da[:, t] = np.concatenate([dar, daz, dan], 1)
            dh = dh + db @ whh
            dwhh += db.T @ hp
        g[f"weight_ih_l{k}"] = da.reshape(-1, 3 * H).T @ inp.reshape(-1, inp.shape[2])
        g[f"weight_hh_l{k}"] = dwhh
        dY = da @ wih
    return dY, flat_weights(g, I, H, N, O)


def last_only_dout(dlast, L):
    """[B, O'] at position L - 1 -> the full [B, L, O'] gradient, zero elsewhere."""
    d = np.zeros((dlast.shape[0], L, dlast.shape[1]))
    d[:, L - 1] = dlast
    return d


def bpr(s, pos, neg):
    """loss = mean_b -log(sigmoid(s . pos - s . neg) + 1e-10); returns (loss, ds, dpos, dneg)."""
    s, pos, neg = (np.asarray(v, np.float64) for v in (s, pos, neg))
    diff = (s * pos).sum(-1) - (s * neg).sum(-1)
    sg = sigmoid(diff)
    loss = float(np.mean(-np.log(sg + 1e-10)))
    dd = (-(sg * (1 - sg)) / (sg + 1e-10) / s.shape[0])[:, None]
    return loss, dd * (pos - neg), dd * s, -dd * s
